"""Randomised cross-check of the ILRA kernels (csrc/ilra.hip) against float64 torch on the CPU: the pooling and the row map through
``ilra_pool_bags`` / ``ilra_rowmap_bags`` (Z, dE, the six row-map gradients, dX, the mask within its band) and, every fourth draw, the
module with 1..3 blocks against the restatement under the kernel's ReLU decisions.  Per draw: 1..12 bags (64 once in a while) of
{1, 2, 7, 15, 16, 17, 31, 32, 33, 255, 256, 257, 300} rows, bf16 / fp32 bag rows or packed fp32 rows with or without a gradient, a row
stride of 512 or 1024, 1..16 queries, as a list or a ``BagSet``.  Gates and measures are the tests' own (tests/ilra_helpers.py), and so
is the precondition on a module's inputs: parameters on which plain fp32 torch on the CPU is itself more than a quarter of the gate from
float64 (three blocks of doubled weights can take the logits to 1e4) are redrawn from the next seed, and more than 10 % redraws fail.
python tools/fuzz_ilra.py [draws] [seed]"""
import os, sys, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import numpy as np
import torch
import ilra_cases as IC
import ilra_edge_cases as EC
import ilra_helpers as IH

draws = int(sys.argv[1]) if len(sys.argv) > 1 else 32
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 96
dev = torch.device("cuda", 0)
SIZES = [1, 2, 7, 15, 16, 17, 31, 32, 33, 255, 256, 257, 300]


def draw(s):
    rng = random.Random(s)
    B = 64 if rng.random() < 0.08 else rng.randint(1, 12)
    sizes = tuple(rng.choice(SIZES[:9] if B == 64 else SIZES) for _ in range(B))          # 64 bags: short ones, the float64 side stays small
    src = rng.choice(["bf16", "f32", "act"])
    return sizes, src, rng.choice([512, 1024]), rng.random() < 0.5, rng.randint(1, 16), rng.random() < 0.5, rng.randint(1, 3)


redrawn = 0
for i in range(draws):
    s = seed + i
    sizes, src, stride, as_set, P, xgrad, L = draw(s)
    tag = f"fuzz seed={s} B={len(sizes)} rows={sum(sizes)} {src} stride={stride} P={P} {'BagSet' if as_set else 'list'} xp.grad={xgrad and src == 'act'}"
    for kind in ("pool", "rowmap"):
        case = EC.EdgeCase(f"{tag} {kind}", "fuzz", kind, sizes, src, P if kind == "pool" else 0, stride, 1.0, "random",
                           None if kind == "pool" else IC.BAND, xgrad and src == "act", 100000 + 17 * s)
        inp = EC.make_inputs(case)
        IH.check_case(case, inp, IH.run_case(case, inp, dev=dev, as_set=as_set))
    if i % 4 == 3:
        rows = "f32" if src == "f32" else "bf16"
        xs = [IC.make_bag(n, rows, 300000 + 64 * s + b) for b, n in enumerate(sizes)]
        w = np.random.RandomState(s).standard_normal((len(xs), 4)).astype(np.float32)
        pseed = 200000 + s
        while True:
            params = IC.make_params(L, 4, pseed)
            yard = IH.module_fp32_error(xs, params, L, w)
            if yard <= IH.TOL / 4:
                break
            redrawn += 1
            print(f"[ilra {tag} module L={L}] fp32 on the CPU is {yard:.1e} from float64 (a quarter of the gate: {IH.TOL / 4:.1e}): parameters redrawn")
            assert redrawn <= 0.1 * draws, ("too many draws redrawn", redrawn, draws)
            pseed += 1000000
        m = IH.build_model(L, 4, params, dev)
        case = EC.EdgeCase(tag, "fuzz", "module", sizes, rows, 8, stride, 1.0, "random", IC.BAND, False, s)
        bags = IH.device_bags(case, {"xs": xs}, dev, as_set=as_set)
        logits, states, grads = IH.run_module(m, bags, w)
        IH.check_module(f"{tag} module L={L}", logits, states, grads, xs, params, L, w)
    print(f"[ilra {tag}] ok")
torch.cuda.synchronize()
print(f"fuzz ilra ok: {draws} draws from seed {seed}, {redrawn} redrawn; worst relative error {IH.WORST[0]:.2e} (gate {IH.TOL:.0e})")
