"""MaxMIL over a batch of bags on the GPU: the batched routes (``VF.max_pool_bags``; behind a trainable Feat_Projecter
``VF.project_max_pool_bags``, the selected-row route) against the routes they replace, which stay in the tree: ``VF.colmax`` bag by
bag for the forward, and for training the projected rows pooled by torch's ``amax`` bag by bag.

Forward (no gradient), bf16 rows: 64 bags x 50 000 rows, 64 x 2 798, 256 x 2 798, and one 2 798-row bag per call.  Training (forward +
backward, DeepMIL(pooling='max', use_feat_proj=True), Linear head): 64 x 2 798 and 64 x 50 000; ``dense`` is the batched projecter
node followed by ``VF.max_pool_bags`` (row gradients of all bags in one launch), ``selected`` what ``DeepMIL.forward_bags`` runs.

Timing: every call sits between two device events; 5 warm-up calls per route, then 20 timed calls per route with the routes taking
turns call by call in one process; the median of the 20.  The whole comparison is repeated ``--repeats`` times: ``us_per_bag`` is the
median of the repeats' medians, ``spread`` their minimum and maximum.  Also per route: ``torch.cuda.max_memory_allocated`` over its
calls (MiB, the resident bags included), and for the forward the bag bytes over the time as a share of 8 TB/s.
Prints one JSON line per shape and mode."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vlsa_amd import functional as VF  # noqa: E402
from vlsa_amd.deepmil import DeepMIL  # noqa: E402

HBM_BYTES_PER_S = 8e12
WARMUP, CALLS = 5, 20


def one_call(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def compare(routes, repeats):
    """{route: (median of the repeats' medians, min, max, peak MiB)} -- microseconds per call"""
    peak = {}
    for name, fn in routes.items():
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() / 2 ** 20
    meds = {name: [] for name in routes}
    for _ in range(repeats):
        ts = {name: [] for name in routes}
        for _ in range(CALLS):
            for name, fn in routes.items():
                ts[name].append(one_call(fn))
        for name in routes:
            meds[name].append(statistics.median(ts[name]))
    return {name: (statistics.median(m), min(m), max(m), peak[name]) for name, m in meds.items()}


def report(out, res, B, nbytes=None):
    for name, (med, lo, hi, peak) in res.items():
        out[name] = {"us_per_bag": round(med / B, 3), "spread": [round(lo / B, 3), round(hi / B, 3)], "peak_MiB": round(peak, 1)}
        if nbytes is not None:
            out[name]["share_of_8TBps"] = round(nbytes / (med * 1e-6) / HBM_BYTES_PER_S, 3)
    print(json.dumps(out), flush=True)


def chunks_of(bags):
    s = VF.BagSet(bags)
    return [s.chunk(i, 64) for i in range(0, len(bags), 64)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forward", type=str, nargs="*", default=["64x50000", "64x2798", "256x2798", "1x2798"])
    ap.add_argument("--train", type=str, nargs="*", default=["64x2798", "64x50000"])
    a = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(0)
    made = {}

    def bags_of(shape):
        if shape not in made:
            made.clear()
            B, N = (int(v) for v in shape.split("x"))
            made[shape] = [torch.randn(N, 512, device=dev).bfloat16() for _ in range(B)]
        return made[shape]

    for shape in a.forward:
        bags = bags_of(shape)
        B, N = len(bags), bags[0].shape[0]
        sets = chunks_of(bags)
        routes = {"per_bag_colmax": lambda: torch.stack([VF.colmax(x) for x in bags]),
                  "batched": lambda: torch.cat([VF.max_pool_bags(c) for c in sets])}
        with torch.no_grad():
            assert torch.equal(routes["per_bag_colmax"](), routes["batched"]())
            res = compare(routes, a.repeats)
        report({"op": "maxmil", "mode": "forward", "bags": B, "rows": N}, res, B, nbytes=B * N * 512 * 2)
        del routes, sets

    for shape in a.train:
        bags = bags_of(shape)
        B, N = len(bags), bags[0].shape[0]
        bagset = VF.BagSet(bags)
        m = DeepMIL(512, 256, 4, pooling="max", use_feat_proj=True, pred_head="default").to(dev).train()
        params = list(m.parameters())
        w = torch.randn(B, 4, device=dev)

        def parent():                   # DeepMIL.forward_bags before the batched route: projecter node, then amax bag by bag
            return m.g(torch.stack([x.float().amax(dim=0) for x in m.feat_proj.forward_bags(bagset)]))

        def dense():
            return m.g(VF.max_pool_bags(m.feat_proj.forward_bags(bagset)))

        def selected():
            return m.forward_bags(bagset)

        def train(f):
            def step():
                for p in params:
                    p.grad = None
                (f() * w).sum().backward()
            return step
        grads = {}
        for name, f in (("parent", parent), ("dense", dense), ("selected", selected)):
            train(f)()
            grads[name] = [p.grad.clone() for p in params]
        check = {name: max(float((g - r).abs().max() / r.abs().max()) for g, r in zip(grads[name], grads["dense"]))
                 for name in ("parent", "selected")}
        res = compare({"parent_amax": train(parent), "dense": train(dense), "selected": train(selected)}, a.repeats)
        report({"op": "maxmil", "mode": "forward+backward", "bags": B, "rows": N, "max_rel_grad_diff_vs_dense": check}, res, B)
        del m, params, grads, bagset


if __name__ == "__main__":
    main()
