"""The continuous survival heads: us per call of value + gradient of SurvPLE from (a) the ONE launch ``vlsa_surv_pair_objective``
(``SurvPairObjective(weight_ple=1).value_and_grad``), (b) a vectorised torch restatement on the same device -- the risk matrix as a
broadcast [B, B] comparison, no Python loop, then ``autograd.grad`` -- and, at B = 32 only, (c) the reference-shaped double loop
``R[i, j] = T[j] >= T[i]`` on device labels, one synchronisation per element (3 calls: it is slow).  Then ``CoxSurvEvaluator.compute``
(``c_index`` + ``loss``) against the (b)-shaped torch route for a split: ``-y_hat`` ranked with the all-pairs comparison matrices
and the same broadcast risk matrix, one ``.item()`` per metric.

Sizes: B = 32, 256 and 4096 (the largest batch of the one launch: a single workgroup walks 16.8 M pairs per pass); M = 1000 and 4096.  Timing: wall clock around 20 back-to-back calls with a device synchronisation before and
after, divided by 20; 5 warm-up rounds per route, then 20 such samples per route, the routes taking turns sample by sample in one
process; the median of the 20.  The whole comparison is repeated 3 times: ``us`` is the median of the three medians, ``spread`` their
minimum and maximum.  Prints one JSON line per size.  Information, not a gate."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vlsa_amd.evaluate import CoxSurvEvaluator  # noqa: E402
from vlsa_amd.losses import SurvPairObjective  # noqa: E402

WARMUP, INNER, CALLS, REPEATS = 5, 20, 20, 3
CAP = 10.0


def torch_ple(pred, t, e, R=None):
    theta = torch.where(pred > CAP, torch.full_like(pred, CAP), pred)
    if R is None:
        R = (t.view(1, -1) >= t.view(-1, 1)).to(pred.dtype)
    return -torch.mean((theta - torch.log(torch.sum(torch.exp(theta) * R, dim=1))) * e)


def loop_risk_matrix(t):
    """loss/loss_surv.py:196-199 on device labels: every element is a comparison on the device and a copy to the host"""
    n = len(t)
    R = torch.zeros([n, n], dtype=torch.int8)
    for i in range(n):
        for j in range(n):
            R[i, j] = t[j] >= t[i]
    return R.float().to(t.device)


def torch_cindex(t, e, est, tied_tol=1e-8):
    ev = e != 0
    ti, tj = t.view(-1, 1), t.view(1, -1)
    comp = (ev.view(-1, 1) & (tj > ti)) | (ev.view(-1, 1) & (tj == ti) & ~ev.view(1, -1))
    tied = (est.view(1, -1) - est.view(-1, 1)).abs() <= tied_tol
    con = comp & ~tied & (est.view(1, -1) < est.view(-1, 1))
    return ((con.sum().double() + 0.5 * (comp & tied).sum().double()) / comp.sum().double()).item()


def sample(fn, inner=INNER):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / inner, out


def compare(routes):
    outs = {}
    for name, fn in routes.items():
        for _ in range(WARMUP):
            outs[name] = sample(fn)[1]
    meds = {name: [] for name in routes}
    for _ in range(REPEATS):
        ts = {name: [] for name in routes}
        for _ in range(CALLS):
            for name, fn in routes.items():
                ts[name].append(sample(fn)[0])
        for name in routes:
            meds[name].append(statistics.median(ts[name]))
    return outs, {name: {"us": round(statistics.median(m), 1), "spread": [round(min(m), 1), round(max(m), 1)]} for name, m in meds.items()}


def inputs(n, dev):
    g = torch.Generator().manual_seed(4200 + n)
    pred = (2.0 * torch.randn(n, generator=g)).to(dev)
    t = (torch.randperm(n, generator=g).float() + 0.5 * torch.rand(n, generator=g)).mul(12.0 / n).to(dev)
    e = (torch.rand(n, generator=g) < 0.6).float().to(dev)
    return pred, t, e


def main():
    dev = torch.device("cuda", 0)
    obj = SurvPairObjective(weight_ple=1.0)
    for B in (32, 256, 4096):
        pred, t, e = inputs(B, dev)

        def launch():
            return obj.value_and_grad(pred, t, e)

        def torch_vectorised():
            x = pred.detach().requires_grad_(True)
            loss = torch_ple(x, t, e)
            return loss.detach(), torch.autograd.grad(loss, x)[0]

        outs, line = compare({"one_launch": launch, "torch_vectorised": torch_vectorised})
        dv = abs(outs["one_launch"][0].item() - outs["torch_vectorised"][0].item())
        dg = (outs["one_launch"][1] - outs["torch_vectorised"][1]).abs().max().item()
        assert dv < 1e-4 and dg < 1e-4, (dv, dg)            # the routes time the same objective
        line = dict({"op": "surv_pair_objective", "term": "SurvPLE", "B": B, "value_diff": dv, "grad_diff": dg}, **line)
        if B == 32:
            def reference_loop():
                x = pred.detach().requires_grad_(True)
                loss = torch_ple(x, t, e, loop_risk_matrix(t))
                return loss.detach(), torch.autograd.grad(loss, x)[0]

            times = [sample(reference_loop, inner=1)[0] for _ in range(3)]
            line["reference_loop"] = {"us": round(statistics.median(times), 1), "spread": [round(min(times), 1), round(max(times), 1)], "calls": 3}
        print(json.dumps(line), flush=True)
    for M in (1000, 4096):
        pred, t, e = inputs(M, dev)
        ev = CoxSurvEvaluator()
        data = {"y": torch.stack([t.double(), e.double()], dim=1), "y_hat": pred.view(-1, 1), "uid": None, "name": "test"}

        def evaluator():
            return ev.compute(data, ["c_index", "loss"])

        def torch_route():
            return {"c_index": torch_cindex(t.double(), e, (-pred).double()), "loss": torch_ple(pred.double(), t.double(), e.double()).item()}

        outs, line = compare({"evaluator": evaluator, "torch_route": torch_route})
        assert abs(outs["evaluator"]["c_index"] - outs["torch_route"]["c_index"]) < 1e-12
        assert abs(outs["evaluator"]["loss"] - outs["torch_route"]["loss"]) < 1e-9
        print(json.dumps(dict({"op": "cox_evaluator", "metrics": ["c_index", "loss"], "M": M, "c_index": outs["evaluator"]["c_index"],
                               "loss": outs["evaluator"]["loss"]}, **line)), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU: no timing without one"
    main()
