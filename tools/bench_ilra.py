"""ILRA on the GPU: the HIP route (``vlsa_amd.deepmil.ILRA.forward_bags``) against a batched torch sequence of the same model.

Shapes: 64 bags x 50 000 rows, 256 bags x 2 798 rows, and one 2 798-row bag per call; bf16 rows; forward, and forward + backward.  Per
run: microseconds per bag (median of ``--reps`` windows of back-to-back calls between two events, the routes' windows alternating).

The torch baseline is the model's algebra batched over [B, N, d] tensors with library GEMMs: per block one [B, N, d] x [d, 8] score
product, a softmax over N, one [B, 8, N] x [B, N, d] product, the [B, 256]-sized tail, and for the row map two [B N, d] x [d, 256]
products and one [B N, 256] x [256, 256] -- and autograd's backward.  It already uses the effective queries (it skips the reference's
fc_k / fc_v over the N rows), which favours torch; the rows are stacked OUTSIDE the timed region.  ``torch_f32`` converts the rows to
fp32 (what the HIP route computes), ``torch_bf16`` runs the N-sized products in bf16, which is cheaper and coarser.  Before a shape is
timed, the three routes' logits are compared at that shape with the same sequence in float64 (on 4 of the bags).
Prints one JSON line per run."""
import argparse
import contextlib
import io
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vlsa_amd.deepmil import ILRA  # noqa: E402


def torch_route(m, X, big):
    """logits [B, num_cls] of X [B, N, 512]; big: the dtype of the N-sized products; the tails in fp32 (float64 for big = float64)"""
    small = torch.float64 if big == torch.float64 else torch.float32
    c = lambda t: t.to(small)          # noqa: E731
    X = X.to(big)

    def block(mha, seed, X, gated):
        a = mha.multihead_attn
        Wi, bi = c(a.in_proj_weight), c(a.in_proj_bias)
        qf = F.linear(c(seed).view(1, 256), c(mha.fc_q.weight), c(mha.fc_q.bias))[0]
        qp = F.linear(qf, Wi[:256], bi[:256])
        E = (qp.view(8, 32, 1) * (Wi[256:512] @ c(mha.fc_k.weight)).view(8, 32, -1)).sum(1) / math.sqrt(32.0)
        A = torch.softmax((X @ E.to(big).t()).float() if big != torch.float64 else X @ E.t(), dim=1).to(big)          # [B, N, 8]
        Z = (A.transpose(1, 2) @ X).to(small)                                                                          # [B, 8, d]
        v = F.linear(F.linear(Z, c(mha.fc_v.weight), c(mha.fc_v.bias)), Wi[512:], bi[512:])
        B = v.shape[0]
        O = qf[None] + F.linear(v.view(B, 8, 8, 32).diagonal(dim1=1, dim2=2).permute(0, 2, 1).reshape(B, 256), c(a.out_proj.weight),
                                c(a.out_proj.bias))
        O = O + torch.relu(F.linear(O, c(mha.fc_o.weight), c(mha.fc_o.bias)))
        if gated:
            g = mha.gate[0]
            O = O * F.silu(F.linear(c(seed).view(1, 256), c(g.weight), c(g.bias)))
        return O

    for blk in m.gab_blocks:
        H = block(blk.project_forward, blk.latent, X, True)
        pb = blk.project_backward
        a = pb.multihead_attn
        cb = F.linear(F.linear(F.linear(H, c(pb.fc_v.weight), c(pb.fc_v.bias)), c(a.in_proj_weight)[512:], c(a.in_proj_bias)[512:]),
                      c(a.out_proj.weight), c(a.out_proj.bias))
        u = F.linear(X, pb.fc_q.weight.to(big)) + (c(pb.fc_q.bias)[None] + cb).to(big)[:, None, :]
        o = u + torch.relu(F.linear(u, pb.fc_o.weight.to(big), pb.fc_o.bias.to(big)))
        X = o * F.silu(F.linear(X, pb.gate[0].weight.to(big), pb.gate[0].bias.to(big)))
    feat = block(m.pooling.mha, m.pooling.S, X, False)
    return F.linear(feat, c(m.classifier.weight), c(m.classifier.bias)).float()


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def timed(fns, inner, reps):
    for fn in fns.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ts[name].append(window(fn, inner))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", type=str, nargs="+", default=["64x50000", "256x2798", "1x2798"])
    a = ap.parse_args()
    dev = "cuda"
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = ILRA(dim_in=512, dim_hid=256, num_cls=4, num_layers=2).to(dev)
    with torch.no_grad():          # the "live" recipe of the tests: the default initialisation cannot tell one bag from another
        for k, p in m.named_parameters():
            if k.endswith("bias"):
                p.uniform_(-0.05, 0.05)
            elif not k.startswith("classifier"):
                p.mul_(2.0)
    params = list(m.parameters())
    for shape in a.shapes:
        B, N = (int(v) for v in shape.split("x"))
        X = (4 * F.normalize(torch.randn(B, N, 512, device=dev), dim=2)).bfloat16()
        bags = list(X.unbind(0))
        w = torch.randn(B, 4, device=dev)
        routes = {"hip": lambda: m.forward_bags(bags), "torch_f32": lambda: torch_route(m, X, torch.float32),
                  "torch_bf16": lambda: torch_route(m, X, torch.bfloat16)}

        def train(f):
            def step():
                for p in params:
                    p.grad = None
                (f() * w).sum().backward()
            return step
        with torch.no_grad():
            ref = torch_route(m, X[:4], torch.float64).double()
            check = {"bags": B, "rows": N, "max_abs_logit": float(ref.abs().max())}
            check["hip_vs_float64"] = float((m.forward_bags(bags[:4]).double() - ref).abs().max())
            check["torch_f32_vs_float64"] = float((torch_route(m, X[:4], torch.float32).double() - ref).abs().max())
            check["torch_bf16_vs_float64"] = float((torch_route(m, X[:4], torch.bfloat16).double() - ref).abs().max())
        print(json.dumps({"op": "ilra", "check": check}), flush=True)
        for mode in ("forward", "forward+backward"):
            out = {"op": "ilra", "mode": mode, "bags": B, "rows": N}
            if mode == "forward":
                with torch.no_grad():
                    ts = timed(routes, a.inner, a.reps)
            else:
                ts = timed({name: train(f) for name, f in routes.items()}, a.inner, a.reps)
            for name, t in ts.items():
                out[name + "_us_per_bag"] = round(t[0] / B, 2)
                out[name + "_min_max_us"] = [round(t[1] / B, 2), round(t[2] / B, 2)]
            print(json.dumps(out), flush=True)
        del X, bags, routes


if __name__ == "__main__":
    main()
