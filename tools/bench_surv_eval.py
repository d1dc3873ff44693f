"""Scoring a split: ``vlsa_amd.evaluate.SurvEvaluator.compute`` from the device logits (two launches, its one device-to-host copy
included) against what the tree did for the same numbers before it: ``.cpu()``, torch softmax, ``oracle.concordance_index`` (a Python
loop over the events) and ``oracle.surv_ifmle``.  Incidence predictions, metrics ``c_index`` + ``loss``.

Shapes (M, K): (1000, 4), (257, 12), (4096, 12).  Timing: wall clock around each call with a device synchronisation before and after
(the host route is host work; the device route ends in its copy); 3 warm-up calls per route, then 20 timed calls per route, the routes
taking turns call by call in one process; the median of the 20.  The whole comparison is repeated 3 times: ``us`` is the median of the
three medians, ``spread`` their minimum and maximum.  ``device_launches_us`` is the time between two device events around
``compute_device`` (the label conversions and the two launches, no copy).  Prints one JSON line per shape, with the two routes' C and
loss (float64 rows against fp32 ones)."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import vlsa_oracle as O  # noqa: E402
from vlsa_amd.evaluate import SurvEvaluator  # noqa: E402

SHAPES = [(1000, 4), (257, 12), (4096, 12)]
WARMUP, CALLS, REPEATS = 3, 20, 3


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6, out


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    dev = torch.device("cuda", 0)
    ev = SurvEvaluator("incidence")
    for M, K in SHAPES:
        g = torch.Generator().manual_seed(M + K)
        logits = (1.5 * torch.randn(M, K, generator=g)).to(dev)
        t = torch.randint(0, K, (M,), generator=g)
        e = (torch.rand(M, generator=g) < 0.6).float()
        e[(e == 0) & (t == K - 1)] = 1.0
        y = torch.stack([t.float(), e], dim=1).to(dev)
        data = {"y": y, "raw_y_hat": logits}

        def device_route():
            return ev.compute(data, ["c_index", "loss"])

        def host_route():
            yc, inc = y.cpu(), torch.softmax(logits.cpu(), dim=-1)
            return {"c_index": O.concordance_index(yc, inc), "loss": float(O.surv_ifmle(inc, yc[:, 0], yc[:, 1]))}

        routes = {"device": device_route, "host": host_route}
        outs = {}
        for name, fn in routes.items():
            for _ in range(WARMUP):
                outs[name] = fn()
        meds = {name: [] for name in routes}
        for _ in range(REPEATS):
            ts = {name: [] for name in routes}
            for _ in range(CALLS):
                for name, fn in routes.items():
                    ts[name].append(wall(fn)[0])
            for name in routes:
                meds[name].append(statistics.median(ts[name]))
        launches = statistics.median(events(lambda: ev.compute_device(data, ["c_index", "loss"])) for _ in range(CALLS))
        line = {"op": "surv_eval", "M": M, "K": K, "device_launches_us": round(launches, 1)}
        for name in routes:
            line[name] = {"us": round(statistics.median(meds[name]), 1), "spread": [round(min(meds[name]), 1), round(max(meds[name]), 1)],
                          "c_index": outs[name]["c_index"], "loss": outs[name]["loss"]}
        line["pairs"] = ev.counts["comparable"]
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
