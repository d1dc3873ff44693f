"""DeepAttnMISL's cluster layer (phi + per-cluster mean) on the GPU: the HIP route against the same op sequence from torch library calls.

Runs forward, and forward + backward, at 2 798 and 50 000 bf16 rows, one bag and 64 bags per call.  Per run: microseconds per bag
(median of ``--reps`` windows of back-to-back calls between two events, the routes' windows alternating) and the share of the bf16 MFMA peak the ALGORITHMIC FLOP
make (2 x 512 x 256 per row forward, twice that more for the backward's dWp; the split terms the kernel really issues are not counted).

The torch baseline is the batched formulation: ONE [sum N, 512] x [512, 256] GEMM with bias over the bags' concatenated rows, relu,
one index_add_ into [B Kc, 256] with the ids offset by Kc per bag, a bincount, a division -- and autograd's backward.  The rows are
concatenated and the ids offset OUTSIDE the timed region (the HIP route reads the bags where they lie), which favours torch.  Two
precisions of it: ``torch_f32`` converts the rows to fp32 and runs the GEMM on the fp32 weights -- what the HIP route computes --,
``torch_bf16`` rounds weights, bias and activations to bf16, which is cheaper and coarser.  Before a size is timed the three routes'
outputs and gradients are compared at that size with the same sequence in float64 (gradients relative to the tensor's largest entry).
The gradient is discontinuous in the ReLU decisions: one decision taken the other way at |pre| ~ 1e-8 moves dWp by that row's dS x,
which among millions of rows with random upstream gradients is ~1e-3 of the largest entry.  So the HIP route, whose decisions can be
read, is also compared with the float64 sequence TAKING ITS DECISIONS, and the run stops if that comparison is more than 1e-4 off; the
number of its decisions that differ from float64's, and the largest |pre| among them, are printed.
Prints one JSON line per run."""
import argparse
import json
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vlsa_amd import functional as VF  # noqa: E402

PEAK = 2.5e15      # dense bf16 MFMA, FLOP/s
TOL = 1e-4


def torch_route(X, cid, W, b, rows, low, acc=torch.float32, mask=None):
    """X [sum N, 512] bf16, cid [sum N] = Kc * bag + id, rows = B * Kc; low: the GEMM in bf16; acc: the type of the sums; mask: ReLU
    decisions to take instead of pre > 0"""
    if low:
        pre = torch.nn.functional.linear(X, W.to(X.dtype), b.to(X.dtype)).float()
    else:
        pre = torch.nn.functional.linear(X.to(W.dtype), W, b)
    h = torch.relu(pre) if mask is None else pre * mask
    s = torch.zeros(rows, 256, device=X.device, dtype=acc).index_add_(0, cid, h)
    return s / torch.bincount(cid, minlength=rows).clamp(min=1)[:, None]


def err(r, ref):
    """hc absolute, the gradients relative to the tensor's largest entry"""
    return {"hc_max_abs": float((r[0] - ref[0]).abs().max()), "dW_max_rel": float((r[1] - ref[1]).abs().max() / ref[1].abs().max()),
            "db_max_rel": float((r[2] - ref[2]).abs().max() / ref[2].abs().max())}


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / inner          # microseconds per call


def timed(fns, inner, reps, min_window_us=20e3):
    """name -> (median, min, max) microseconds per call.  Every route is warmed up, given as many calls per window as make the window
    at least ``min_window_us`` long (never fewer than ``inner``), and the routes' windows ALTERNATE, so that a drift of the machine
    lands on all of them alike."""
    n = {}
    for name, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        n[name] = max(inner, min(2000, int(min_window_us / max(window(fn, inner), 1e-3)) + 1))
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ts[name].append(window(fn, n[name]))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in ts.items()}, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2798, 50000])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64])
    a = ap.parse_args()
    dev, Kc = "cuda", 8
    torch.manual_seed(0)
    W = (torch.randn(256, 512, device=dev) / 512 ** 0.5).requires_grad_(True)
    b = (torch.randn(256, device=dev) * 0.05).requires_grad_(True)
    for N in a.sizes:
        for B in a.batches:
            bags = [torch.nn.functional.normalize(torch.randn(N, 512, device=dev), dim=1).bfloat16() for _ in range(B)]
            idss = [torch.randint(0, Kc, (N,), device=dev) for _ in range(B)]
            g = torch.randn(B, Kc, 256, device=dev)
            X, cid = torch.cat(bags), torch.cat([c + Kc * i for i, c in enumerate(idss)])
            routes = {"hip": lambda: VF.cluster_pool_bags(bags, idss, W, b, num_clusters=Kc),
                      "torch_f32": lambda: torch_route(X, cid, W, b, B * Kc, False).view(B, Kc, 256),
                      "torch_bf16": lambda: torch_route(X, cid, W, b, B * Kc, True).view(B, Kc, 256)}

            def train(f, dhc=g):
                def step():
                    W.grad = b.grad = None
                    f().backward(dhc)
                return step
            # the outputs at the size that is timed, against the same sequence in float64
            def run(f, dhc=g):
                train(f, dhc)()
                return f().detach().double(), W.grad.double(), b.grad.double()

            def f64(mask=None):
                return lambda: torch_route(X, cid, W.double(), b.double(), B * Kc, False, torch.float64, mask).view(B, Kc, 256)
            ref = run(f64(), g.double())
            check = {"rows": N, "bags": B}
            for name in ("torch_f32", "torch_bf16"):
                check[name + "_vs_float64"] = err(run(routes[name]), ref)
            with torch.no_grad():
                words = VF.cluster_pool_bags(bags, idss, W, b, num_clusters=Kc, ret_state=True)[2]
                taken = ((words[:, :, None] >> torch.arange(32, device=dev, dtype=torch.int32)) & 1).reshape(-1, 256).bool()
                pre = torch.nn.functional.linear(X.double(), W.double(), b.double())
                differ = taken != (pre > 0)
                check["hip_relu_decisions_differing_from_float64"] = [int(differ.sum()), float(pre[differ].abs().max()) if bool(differ.any()) else 0.0]
                del words, pre, differ
            check["hip_vs_float64"] = err(run(routes["hip"]), ref)
            check["hip_vs_float64_taking_its_relu_decisions"] = err(run(routes["hip"]), run(f64(taken), g.double()))
            print(json.dumps({"op": "deepattnmisl_cluster_pool", "check": check}), flush=True)
            if max(check["hip_vs_float64_taking_its_relu_decisions"].values()) > TOL:
                raise SystemExit(f"the HIP route and the float64 sequence differ by more than {TOL} at {N} rows x {B} bags")
            del ref, taken
            for mode, flop in (("forward", 2 * 512 * 256), ("forward+backward", 3 * 2 * 512 * 256)):
                out = {"op": "deepattnmisl_cluster_pool", "mode": mode, "rows": N, "bags": B}
                if mode == "forward":
                    with torch.no_grad():
                        ts, n = timed(routes, a.inner, a.reps)
                else:
                    ts, n = timed({name: train(f) for name, f in routes.items()}, a.inner, a.reps)
                for name, t in ts.items():
                    out[name + "_us_per_bag"] = round(t[0] / B, 2)
                    out[name + "_min_max_us"] = [round(t[1] / B, 2), round(t[2] / B, 2)]
                    out[name + "_share_of_bf16_peak"] = round(flop * N * B / (t[0] * 1e-6) / PEAK, 4)
                    out[name + "_calls_per_window"] = n[name]
                print(json.dumps(out), flush=True)
            del bags, idss, X, cid, routes


if __name__ == "__main__":
    main()
