"""Feat_Projecter over a batch of bags: the per-bag loop (``[m(x) for x in bags]``: one launch, one allocation and -- when the
projecter trains -- one autograd node with its own dW per bag) against ``m.forward_bags(bags)`` (one launch into one packed
allocation per chunk of 64 bags, one autograd node, one dW), in ONE process, the two alternating.

    python tools/bench_featproj_bags.py [--legs tcga,50k] [--rounds 5] [--reps 10] [--bagset]

Legs: ``tcga`` = 32 bags of 2 000 - 12 000 rows (bench.py's seed-0 list), ``50k`` = 32 bags of 50 000 rows; bf16 and fp32 each;
``fwd`` = inference forward under no_grad, ``fwd+bwd`` = training forward and the backward of the projecter alone (the gradient
of sum_i <Y_i, G_i> with fixed G_i: the downstream node is two packed reads, the same for both routes).  Device-event times of
``reps`` calls, best of ``rounds`` rounds per route with the routes alternating inside a round; one JSON line per leg at the end."""
import argparse
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from vlsa_amd import functional as VF  # noqa: E402
from vlsa_amd.layers import Feat_Projecter  # noqa: E402


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def alternate(fns: dict, rounds, reps):
    for fn in fns.values():                            # warm-up: code objects, allocator segments, packed weights
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, reps))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="tcga,50k")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--bagset", action="store_true", help="hand forward_bags a BagSet (tables derived on the device, kept with the set)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    gc.collect()
    gc.freeze()
    sizes = {"tcga": [int(x) for x in torch.randint(2000, 12000, (32,), generator=torch.Generator().manual_seed(0))],
             "50k": [50000] * 32}
    torch.manual_seed(0)
    m = Feat_Projecter(512, 512).to(dev)
    results = []
    for leg in args.legs.split(","):
        for dtype in (torch.bfloat16, torch.float32):
            torch.cuda.empty_cache()
            g = torch.Generator(device=dev).manual_seed(1)
            bags = [torch.randn(n, 512, device=dev, generator=g).to(dtype) for n in sizes[leg]]
            G = torch.randn(sum(sizes[leg]), 512, device=dev, generator=g)
            Gs = list(G.split(sizes[leg]))
            batch_in = VF.BagSet(bags) if args.bagset else bags

            def loop_fwd():
                with torch.no_grad():
                    return [m(x) for x in bags]

            def batch_fwd():
                with torch.no_grad():
                    return m.forward_bags(batch_in)

            def train(ys):
                m.zero_grad(set_to_none=True)
                torch.autograd.backward(ys, Gs)

            # the two routes give the same rows (bit for bit) and the same gradients up to the order of the cross-bag sum
            assert all(torch.equal(a, b) for a, b in zip(loop_fwd(), batch_fwd()))
            train([m(x) for x in bags])
            ref = m.projecter[0].weight.grad.clone()
            train(m.forward_bags(batch_in))
            dw_err = ((m.projecter[0].weight.grad - ref).abs().max() / ref.abs().max()).item()
            t = alternate({"loop fwd": loop_fwd, "batch fwd": batch_fwd,
                           "loop fwd+bwd": lambda: train([m(x) for x in bags]),
                           "batch fwd+bwd": lambda: train(m.forward_bags(batch_in))}, args.rounds, args.reps)
            r = {"leg": leg, "dtype": str(dtype)[6:], "bags": len(bags), "rows": sum(sizes[leg]), "bagset": bool(args.bagset),
                 "dW_rel_diff": dw_err}
            for k, v in t.items():
                r[k + " us"] = round(min(v), 1)
                r[k + " spread"] = round((max(v) - min(v)) / min(v), 3)
            r["fwd speedup"] = round(r["loop fwd us"] / r["batch fwd us"], 3)
            r["fwd+bwd speedup"] = round(r["loop fwd+bwd us"] / r["batch fwd+bwd us"], 3)
            results.append(r)
            print(json.dumps(r), flush=True)
            del bags, G, Gs, batch_in
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "results": results}))


if __name__ == "__main__":
    main()
