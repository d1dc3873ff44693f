"""Randomised cross-check of the DSMIL kernels (csrc/dsmil.hip) against torch on the CPU: the collapsed formula in float64 with the
dropout masks restated in Python (tests/dsmil_helpers.py), forward and backward.  Per draw: C uniform in 1..16, fp32 or bf16 rows,
1..12 ragged bags of up to 3000 rows sized around the multiples of 32, 64 and 512 (+-2), with or without dropout, as a list or a
``BagSet`` through ``DSMIL.forward_bags``.  Gates and the precondition on the argmax are the tests' own (dsmil_helpers.check_forward /
check_grads / MARGIN); a draw whose bags leave a critical row open is redrawn from the next seed, and more than 10 % redraws fail.
python tools/fuzz_dsmil.py [draws] [seed]"""
import os, sys, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import numpy as np
import torch
import dsmil_cases as DC
import dsmil_helpers as DH
from vlsa_amd import functional as F

draws = int(sys.argv[1]) if len(sys.argv) > 1 else 40
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 28
dev = torch.device("cuda", 0)


def draw(s):
    rng = random.Random(s)
    C, kind, B = rng.randint(1, 16), rng.choice(["f32", "bf16"]), rng.randint(1, 12)
    sizes = []
    for _ in range(B):
        if rng.random() < 0.7:
            u = rng.choice([32, 64, 512])
            sizes.append(min(3000, max(1, u * rng.randint(1, 3000 // u) + rng.randint(-2, 2))))
        else:
            sizes.append(rng.randint(1, 3000))
    p = rng.choice([0.1, 0.25, 0.5]) if rng.random() < 0.5 else 0.0
    return C, kind, sizes, p, rng.random() < 0.5


done = redrawn = 0
s = seed
while done < draws:
    C, kind, sizes, p, as_set = draw(s)
    tag = f"fuzz seed={s} C={C} {kind} p={p} {'BagSet' if as_set else 'list'}"
    xs = [DC.make_rows(n, kind, s * 100 + i) for i, n in enumerate(sizes)]
    params = DC.make_params(C, s, False, 8.0)
    P = [torch.from_numpy(params[k]) for k in DC.KEYS]
    s += 1
    if min(DH.score_margin(torch.from_numpy(x), P) for x in xs) < DH.MARGIN:
        redrawn += 1
        print(f"[dsmil {tag}] a critical row is open (float64 margin below {DH.MARGIN:.0e}): redrawn")
        assert redrawn <= 0.1 * draws, ("too many draws redrawn", redrawn, draws)
        continue
    G = np.random.RandomState(s).standard_normal((len(xs), C))
    word = 1000003 + 7 * s
    m = DH.build_model(C, s - 1, dev, drop=p, q_scale=8.0)
    if p:
        m.train()
        m._drop_counter = torch.tensor([word - 1], dtype=torch.int64, device=dev)       # the call advances it to word
    bags = [torch.from_numpy(x).to(torch.float32 if kind == "f32" else torch.bfloat16).to(dev) for x in xs]
    logits, attn, crit = m.forward_bags(F.BagSet(bags) if as_set else bags, ret_with_attn=True, ret_critical=True)
    (logits * torch.from_numpy(G).float().to(dev)).sum().backward()
    rs = []
    for b, x in enumerate(xs):
        mask = DH.keep_mask(word, b, x.shape[0], p) if p else None
        r = DH.torch_case(torch.from_numpy(x), P, [G[b:b + 1]], formula=DH.collapsed_formula, mask=mask, p=p)
        DH.check_forward(f"{tag} bag {b} N={sizes[b]}", logits[b:b + 1].detach(), attn[b], crit[b], DH.case_ref(r))
        rs.append(r)
    DH.check_grads(tag, [t.grad for t in DH.module_params(m)],
                   DH.grad_ref(DH.sum_grads([r["grads"][0] for r in rs]), DH.sum_grads([r["grads32"][0] for r in rs])))
    done += 1
torch.cuda.synchronize()
print(f"fuzz dsmil ok: {done} draws from seed {seed}, {redrawn} redrawn; worst (error, gate)", DH.WORST)
