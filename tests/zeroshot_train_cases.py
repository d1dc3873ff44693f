"""Cases of the differentiable zero-shot route (identity FeatMIL + logit pooling with trainable text features), shared by
tests/test_zeroshot_train_cpu.py and tests/test_gpu_zeroshot_train.py: the batches, the float64 reference (the oracle under autograd,
on the bf16-rounded values for bf16 bags), a numpy restatement of the closed-form gradient, and the selection-gap precondition.

A near-tie at the k-th place of a (bag, class) row makes the selected set -- and so the gradient -- ill-defined, so every top-k case
asserts that the k-th and (k+1)-th float64 cosines differ by >= GAP.  The text features' seed of each case (SEEDS) was searched so that
EVERY case meets it; ``find_seed`` is the search (run this file as a script to redo the table after changing a batch)."""
import functools

import numpy as np
import torch

import cases
from oracle import vlsa_oracle as O

GAP = 1e-4
POOLINGS = ("logit_max", "logit_top3", "logit_top10", "logit_mean")
RAGGED = (1, 5, 10, 11, 257, 2798)          # below, at and above k = 10; one row; one that does not divide a tile
BATCHES = {"ragged": RAGGED, "one": (37,), "b65": tuple(12 + (7 * i) % 29 for i in range(65))}      # b65 crosses the 64-bag chunk
# (batch, K): 18 classes cross the MAX_P = 16 class chunk
SHAPES = [("ragged", 4), ("ragged", 12), ("ragged", 18), ("one", 4), ("b65", 4)]
DTYPES = ("bf16", "fp32")
CASES = [(b, K, dt, p) for b, K in SHAPES for dt in DTYPES for p in POOLINGS]


def topk_of(pooling):
    if pooling == "logit_mean":
        return None
    return 1 if pooling == "logit_max" else int(pooling[len("logit_top"):])


@functools.lru_cache(maxsize=None)
def bags_of(batch, dt):
    """the batch's bags as the GPU sees them (fp32, or rounded to bf16), on the CPU"""
    base = {"ragged": 8100, "one": 8200, "b65": 8300}[batch]
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    return tuple(cases.make_bag(n, base + i, "iid").to(dtype) for i, n in enumerate(BATCHES[batch]))


def text_of(K, seed):
    return torch.randn(K, 512, generator=cases.gen(seed))


def upstream_of(B, K, seed):
    return torch.randn(B, K, generator=cases.gen(seed + 1))


def min_gap(bags, T, k):
    """smallest difference between the k-th and (k+1)-th largest float64 cosine over every (bag, class) with N > k"""
    Tn = O.l2_normalize(T.double())
    worst = float("inf")
    for X in bags:
        if X.shape[0] <= k:
            continue
        c = torch.sort(Tn @ O.l2_normalize(X.double()).t(), dim=1, descending=True).values
        worst = min(worst, float((c[:, k - 1] - c[:, k]).min()))
    return worst


def find_seed(batch, K, dt, pooling, start=0, tries=20000):
    k = topk_of(pooling)
    base = 9000 + 1000 * SHAPES.index((batch, K))
    if k is None:
        return base
    for s in range(start, tries):
        if min_gap(bags_of(batch, dt), text_of(K, base + s), k) >= GAP:
            return base + s
    raise RuntimeError("no seed found")


SEEDS = {
    ('ragged', 4, 'bf16', 'logit_max'): 9000,
    ('ragged', 4, 'bf16', 'logit_top3'): 9000,
    ('ragged', 4, 'bf16', 'logit_top10'): 9000,
    ('ragged', 4, 'bf16', 'logit_mean'): 9000,
    ('ragged', 4, 'fp32', 'logit_max'): 9000,
    ('ragged', 4, 'fp32', 'logit_top3'): 9000,
    ('ragged', 4, 'fp32', 'logit_top10'): 9000,
    ('ragged', 4, 'fp32', 'logit_mean'): 9000,
    ('ragged', 12, 'bf16', 'logit_max'): 10000,
    ('ragged', 12, 'bf16', 'logit_top3'): 10003,
    ('ragged', 12, 'bf16', 'logit_top10'): 10000,
    ('ragged', 12, 'bf16', 'logit_mean'): 10000,
    ('ragged', 12, 'fp32', 'logit_max'): 10000,
    ('ragged', 12, 'fp32', 'logit_top3'): 10000,
    ('ragged', 12, 'fp32', 'logit_top10'): 10000,
    ('ragged', 12, 'fp32', 'logit_mean'): 10000,
    ('ragged', 18, 'bf16', 'logit_max'): 11001,
    ('ragged', 18, 'bf16', 'logit_top3'): 11000,
    ('ragged', 18, 'bf16', 'logit_top10'): 11008,
    ('ragged', 18, 'bf16', 'logit_mean'): 11000,
    ('ragged', 18, 'fp32', 'logit_max'): 11001,
    ('ragged', 18, 'fp32', 'logit_top3'): 11000,
    ('ragged', 18, 'fp32', 'logit_top10'): 11014,
    ('ragged', 18, 'fp32', 'logit_mean'): 11000,
    ('one', 4, 'bf16', 'logit_max'): 12000,
    ('one', 4, 'bf16', 'logit_top3'): 12000,
    ('one', 4, 'bf16', 'logit_top10'): 12001,
    ('one', 4, 'bf16', 'logit_mean'): 12000,
    ('one', 4, 'fp32', 'logit_max'): 12000,
    ('one', 4, 'fp32', 'logit_top3'): 12000,
    ('one', 4, 'fp32', 'logit_top10'): 12001,
    ('one', 4, 'fp32', 'logit_mean'): 12000,
    ('b65', 4, 'bf16', 'logit_max'): 13004,
    ('b65', 4, 'bf16', 'logit_top3'): 13005,
    ('b65', 4, 'bf16', 'logit_top10'): 13226,
    ('b65', 4, 'bf16', 'logit_mean'): 13000,
    ('b65', 4, 'fp32', 'logit_max'): 13004,
    ('b65', 4, 'fp32', 'logit_top3'): 13015,
    ('b65', 4, 'fp32', 'logit_top10'): 13419,
    ('b65', 4, 'fp32', 'logit_mean'): 13000,
}


def reference(batch, K, dt, pooling):
    """float64 logits [B, K], dT [K, 512], d logit_scale of L = sum(logits * G) from the oracle under autograd"""
    return _reference(batch, K, dt, pooling)


@functools.lru_cache(maxsize=None)
def _reference(batch, K, dt, pooling):
    bags = bags_of(batch, dt)
    seed = SEEDS[(batch, K, dt, pooling)]
    T = text_of(K, seed).double().requires_grad_(True)
    ls = torch.tensor(cases.LOGIT_SCALE, dtype=torch.float64, requires_grad=True)
    G = upstream_of(len(bags), K, seed).double()
    logits = torch.cat([O.vlsa_zeroshot_forward(X.double(), T, ls, pooling)[0] for X in bags])
    (logits * G).sum().backward()
    return logits.detach(), T.grad.clone(), ls.grad.clone()


def closed_form(bags, T, ls, G, k):
    """numpy float64 restatement of the route's math: (logits [B, K], dT [K, 512], d logit_scale, idx per bag [K, m_b])"""
    T = np.asarray(T, dtype=np.float64)
    tn = np.maximum(np.linalg.norm(T, axis=1, keepdims=True), 1e-12)
    That, s = T / tn, float(np.exp(ls))
    logits, dThat, idxs = np.zeros((len(bags), T.shape[0])), np.zeros_like(T), []
    for b, X in enumerate(bags):
        X = np.asarray(X, dtype=np.float64)
        Xh = X / np.maximum(np.linalg.norm(X, axis=1, keepdims=True), 1e-12)
        c = That @ Xh.T                                            # [K, N]
        N = X.shape[0]
        m = N if k is None else min(k, N)
        sel = np.stack([np.lexsort((np.arange(N), -c[j]))[:m] for j in range(T.shape[0])])      # descending score, then ascending row
        idxs.append(sel)
        for j in range(T.shape[0]):
            logits[b, j] = s * c[j, sel[j]].mean()
            dThat[j] += s * G[b, j] / m * Xh[sel[j]].sum(0)
    dT = (dThat - (dThat * That).sum(1, keepdims=True) * That) / tn
    return logits, dT, float((np.asarray(G) * logits).sum()), idxs


if __name__ == "__main__":
    for case in CASES:
        print(f"    {case!r}: {find_seed(*case)},", flush=True)
