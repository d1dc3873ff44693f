"""One 32-bag step of the prompt pre-training stage (identity FeatMIL + logit pooling, trainable text features and logit scale): the
bag-by-bag route (``net(x)`` per bag: ``F.normalize`` of the whole bag, a [N, 512] x [512, K] product, ``topk`` and their autograd
nodes -- what ``forward_bags`` did for this stage before it had a batched route) against ``net.forward_bags(bags)`` (the streaming
score kernel over the bag table, one selection launch, one backward launch), in ONE process, the two alternating.

    python tools/bench_zeroshot_train.py [--legs tcga,50k] [--poolings logit_top10,logit_mean] [--rounds 5] [--reps 5]

Legs: ``tcga`` = 32 bf16 bags of 2 000 - 12 000 rows (bench.py's seed-0 list), ``50k`` = 32 bf16 bags of 50 000 rows.  A step is the
forward and the backward of sum(logits * G) with a fixed G [32, K]: gradients for the K = 4 text features and the logit scale.
Device-event times of ``reps`` steps, best of ``rounds`` rounds per route with the routes alternating inside a round.  For
``logit_mean`` the unit-row mean launch (vlsa_unit_mean_batch) is also timed alone: achieved fraction of the HBM peak, recorded, not
gated.  One JSON line per leg and pooling at the end."""
import argparse
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from vlsa_amd import _native as nat, functional as VF  # noqa: E402
from vlsa_amd.vlsa import VLSA  # noqa: E402

HBM_PEAK = 8.0e12      # B/s, MI355X data sheet
K = 4


class Prompts(torch.nn.Module):
    """a trainable text side: K raw text features as a parameter (what a CoOp learner + tower hand the model)"""

    def __init__(self):
        super().__init__()
        self.t = torch.nn.Parameter(torch.randn(K, 512, generator=torch.Generator().manual_seed(3)))

    def forward(self):
        return self.t * 1.0


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def alternate(fns: dict, rounds, reps):
    for fn in fns.values():                            # warm-up: code objects, allocator segments
        for _ in range(2):
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
    ap.add_argument("--poolings", default="logit_top10,logit_mean")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    gc.collect()
    gc.freeze()
    sizes = {"tcga": [int(x) for x in torch.randint(2000, 12000, (32,), generator=torch.Generator().manual_seed(0))],
             "50k": [50000] * 32}
    lib = nat.load()
    results = []
    for leg in args.legs.split(","):
        torch.cuda.empty_cache()
        g = torch.Generator(device=dev).manual_seed(1)
        bags = [torch.randn(n, 512, device=dev, generator=g).to(torch.bfloat16) for n in sizes[leg]]
        bagset = VF.BagSet(bags)
        G = torch.randn(len(bags), K, device=dev, generator=g)
        for pooling in args.poolings.split(","):
            net = VLSA.from_modules(dict(name="FeatMIL", dim_in=512, pooling=pooling), text_provider=Prompts()).to(dev).train()
            params = [net.prompt_adapter.t, net.logit_scale]

            def step(route):
                for p in params:
                    p.grad = None
                if route == "loop":
                    logits = torch.cat([net(x[None])[0] for x in bags])
                else:
                    logits = net.forward_bags(bagset)[0]
                (logits * G).sum().backward()
                return logits.detach(), [p.grad.clone() for p in params]

            la, ga = step("loop")
            lb, gb = step("bags")
            r = {"leg": leg, "pooling": pooling, "dtype": "bfloat16", "bags": len(bags), "rows": sum(sizes[leg]), "K": K,
                 "logits_max_diff": float((la - lb).abs().max()),
                 "dT_rel_diff": float((ga[0] - gb[0]).abs().max() / ga[0].abs().max()),
                 "dls_rel_diff": float((ga[1] - gb[1]).abs().max() / ga[1].abs().max())}
            t = alternate({"loop step": lambda: step("loop"), "forward_bags step": lambda: step("bags")}, args.rounds, args.reps)
            for k, v in t.items():
                r[k + " us"] = round(min(v), 1)
                r[k + " spread"] = round((max(v) - min(v)) / min(v), 3)
            r["speedup"] = round(r["loop step us"] / r["forward_bags step us"], 3)
            if pooling == "logit_mean":
                u = torch.empty(len(bags), 512, device=dev)
                ws = torch.empty(lib.vlsa_unit_mean_workspace_bytes(len(bags)), dtype=torch.uint8, device=dev)
                desc = bagset.desc()

                def unit_mean():
                    nat.check(lib.vlsa_unit_mean_batch(VF._p(desc), len(bags), bagset.dt, 512, VF._p(ws), VF._p(u), VF._stream()), "unit_mean")

                us = min(alternate({"u": unit_mean}, args.rounds, 20)["u"])
                r["unit_mean us"] = round(us, 1)
                r["unit_mean hbm frac"] = round(sum(sizes[leg]) * 512 * 2 / (us * 1e-6) / HBM_PEAK, 4)
            results.append(r)
            print(json.dumps(r), flush=True)
            del net
        del bags, bagset
    print(json.dumps({"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "results": results}))


if __name__ == "__main__":
    main()
