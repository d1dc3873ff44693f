"""DeepMIL training: the per-bag route (``torch.cat([enc(x) for x in bags])`` under autograd) against the batched route
(``DeepMIL.forward_bags``: one autograd node per <= 64 bags), alternating A/B in one process.  Rows: encoder forward + backward and the
full 32-bag optimizer step (TrainStep, eager and graph replay), for 32 bags of 2-12k patches (TCGA-like) and 32 x 50k, bf16 and fp32,
gated and ungated.  One JSON line per case.

    python tools/bench_deepmil_step.py [--reps 20] [--quick] [--only-encoder]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bags(kind, dtype, dev):
    g = torch.Generator().manual_seed(7)
    sizes = [50000] * 32 if kind == "50k" else [int(n) for n in torch.randint(2000, 12001, (32,), generator=g)]
    return [(torch.randn(n, 512, generator=g) * 0.5).to(dtype).to(dev) for n in sizes], sizes


def _time(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="bf16 gated only")
    ap.add_argument("--only-encoder", action="store_true")
    args = ap.parse_args()
    from vlsa_amd import functional as VF
    from vlsa_amd.deepmil import DeepMIL
    from vlsa_amd.losses import SurvObjective
    from vlsa_amd.optim import FusedAdam
    from vlsa_amd.train_step import TrainStep
    from vlsa_amd.vlsa import VLSA
    dev = torch.device("cuda", 0)
    cases = [(k, d, p) for k in ("tcga", "50k") for d in (torch.bfloat16, torch.float32) for p in ("gated_attention", "attention")]
    if args.quick:
        cases = [c for c in cases if c[1] == torch.bfloat16 and c[2] == "gated_attention"]
    for kind, dtype, pooling in cases:
        bags, sizes = _bags(kind, dtype, dev)
        bs = VF.BagSet(bags)
        torch.manual_seed(0)
        enc = DeepMIL(dim_in=512, dim_hid=256, num_cls=512, use_feat_proj=False, drop_rate=0.25, pooling=pooling).to(dev).train()
        G = torch.randn(32, 512, device=dev)

        def per_bag():
            out = torch.cat([enc(x[None]) for x in bags])
            (out * G).sum().backward()

        def batched():
            (enc.forward_bags(bs) * G).sum().backward()

        per_bag(), batched()
        a, b = [], []
        for _ in range(3):                                   # alternating A / B
            a.append(_time(per_bag, max(2, args.reps // 4)))
            b.append(_time(batched, args.reps))
        row = {"case": f"{kind} {str(dtype)[6:]} {pooling}", "rows": sum(sizes), "encoder_fwd_bwd_ms": {"per_bag": min(a), "batched": min(b)},
               "speedup": min(a) / min(b)}
        if not args.only_encoder:
            cfg = dict(name="DeepMIL", dim_in=512, dim_hid=256, num_cls=512, use_feat_proj=False, drop_rate=0.25, pooling=pooling)
            torch.manual_seed(0)
            net = VLSA.from_modules(cfg, pretrained_text_features=torch.randn(4, 512), logit_scale_init=4.0).to(dev).train()
            t = torch.randint(0, 4, (32,), device=dev)
            e = (torch.rand(32, device=dev) < 0.5).float()
            for graph in (False, True):
                opt = FusedAdam([{"params": [p for p in net.parameters() if p.requires_grad], "weight_decay": 0.0}], lr=1e-4)
                ts = TrainStep(net, SurvObjective(), opt, graph=graph)
                for _ in range(4):
                    ts.step(bs, t, e)
                row["step_ms_" + ("replay" if graph else "eager")] = _time(lambda: ts.step(bs, t, e), args.reps)
                row["step_mode_" + ("replay" if graph else "eager")] = ts.describe()["mode"]
                ts.close()
        print(json.dumps(row), flush=True)
        del bags, bs


if __name__ == "__main__":
    main()
