"""Seeded bags for the batched max pooling (vlsa_colmax_batch and what is built on it) with the reference result of each: value and
FIRST maximal row of every column from ``torch.max(x.float(), dim=0)`` on the CPU, which is what the reference's MaxMIL pooling
computes (and whose gradient goes to that row).  ``P`` is the library's ``vlsa_colmax_part_rows()``: a bag of N rows is cut into
clamp(ceil(N / P), 1, 512) parts of contiguous rows, split evenly, so a bag of 2 P rows is the parts [0, P) and [P, 2 P).

Every case is a function of (P, dtype) alone.  ``build`` keeps what it built -- and the references -- per (P, dtype): the tests share
them and leave them unchanged."""
import torch

D = 512
SIZES = ("one", "two", "p_minus_1", "p", "p_plus_1", "two_p_plus_3")
_CACHE = {}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(n, seed, dtype, cols=D):
    return torch.randn(n, cols, generator=_gen(seed)).to(dtype)


def reference(x):
    """(values fp32 [512], first maximal row int32 [512]) of a [N, 512] bag"""
    v, i = torch.max(x.float(), dim=0)
    return v, i.to(torch.int32)


def build(P: int, dtype):
    """{name: (x [N, 512] CPU tensor of ``dtype`` -- ``strided`` is a view with row stride 640 --, (values, rows))}"""
    key = (P, dtype)
    if key in _CACHE:
        return _CACHE[key]
    c = {}
    for i, (name, n) in enumerate(zip(SIZES, (1, 2, P - 1, P, P + 1, 2 * P + 3))):
        c[name] = _rand(max(n, 1), 10 + i, dtype)
    c["slide_2798"] = _rand(2798, 20, dtype)
    c["strided"] = _rand(P + 5, 21, dtype, cols=640)[:, :D]
    x = _rand(2 * P + 3, 22, dtype)
    x[0] = 50.0
    c["max_in_first_row"] = x
    x = _rand(2 * P + 3, 23, dtype)
    x[-1] = 50.0
    c["max_in_last_row"] = x
    x = _rand(2 * P, 24, dtype)                   # parts [0, P) and [P, 2 P): the maximum sits in the last row of part 0 AND
    x[P - 1] = 40.0                               # the first row of part 1 (odd columns: once more, further down part 1)
    x[P] = 40.0
    x[P + 1, 1::2] = 40.0
    c["duplicate_across_parts"] = x
    x = _rand(P + 7, 25, dtype)
    x[:, 3] = 1.5                                 # a constant column
    x[:, 5] = -3e38                               # a column of (nearly) the most negative finite value
    x[:, 6] = float("-inf")                       # a column of -inf
    x[:, 7] = -1.0                                # -0.0 before +0.0 ...
    x[2, 7], x[4, 7] = -0.0, 0.0
    x[:, 8] = -1.0                                # ... and +0.0 before -0.0: a tie either way
    x[2, 8], x[4, 8] = 0.0, -0.0
    c["special_columns"] = x
    out = _CACHE[key] = {k: (v, reference(v)) for k, v in c.items()}
    return out
