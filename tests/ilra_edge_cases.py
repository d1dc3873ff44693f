"""Shapes, strides, query counts and score profiles at which the ILRA kernels (vlsa_amd/csrc/ilra.hip) take another path, and seeded
inputs for them.  tests/test_ilra_edge_cases_cpu.py pins every case to the library's own part / tile / split arithmetic and holds the
inputs to the yardstick (plain fp32 torch on the CPU within a quarter of ``ilra_helpers.TOL`` of float64, by the GPU test's own
measure); tests/test_gpu_ilra_edges.py replays the table on the kernels.  Imports without a GPU.

What the kernels decide from a case's numbers:
    pooling     tiles of 16 rows; a bag owns vlsa_ilra_pool_parts(N) = clamp(ceil(N / 256), 1, 64) parts, part g walks the tiles
                g, g + G, ...: the clamp binds from N = 16385 on (16384 rows: 64 parts of 16 tiles; 16385: the first part walks 17).
                P <= 16 queries: lane i16 owns query i16, register group gq the queries 4 gq .. 4 gq + 3.
    row map     tiles of 32 rows; the weight gradients in splits_of(n) = clamp(ceil(n / 4), 1, 64) splits over n tiles, split s walks
                the tiles s, s + R, ...: the clamp binds from 257 tiles on (N = 8192: 256 tiles, 64 splits of 4; 8193: the first walks 5).
                Column sums of a bag in 8 segments of rows [N s / 8, N (s + 1) / 8): empty ones below N = 8.
    row source  "bf16" / "f32": the bag's own rows [N, 512] read with the tensor's row stride; "act": packed fp32 rows [sum N, 256] of a
                previous row map (the bags supply the sizes only), with or without a gradient of their own.

Score profiles (``order``): "random" as drawn; "rising" rows sorted by query 0's score, so that its running maximum rises on every
tile; "spike" one row (the last: the last tile) whose score for query SPIKE_Q exceeds every other row's by SPIKE_MARGIN, so that the
parts without it merge with weight expf(< -104) = 0 in fp32.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch

import ilra_cases as IC

SPIKE_Q, SPIKE_MARGIN = 1, 120.0

# kind: "pool" | "rowmap";  sizes: rows per bag;  src: row source;  P: queries (0: row map);  stride: elements between two rows of a bag
# tensor (512: contiguous, 1024: a [:, :512] view of a [N, 1024] arena);  gain: multiplier on E;  order: the score profile;
# band: the row map's mask band (None: pooling);  xgrad: packed rows carry a gradient;  seed
EdgeCase = namedtuple("EdgeCase", "name group kind sizes src P stride gain order band xgrad seed")

# name -> mask band, where it has to lie above ilra_cases.BAND: 10 x the largest |t64| at which the CPU's fp32 evaluation flips a ReLU
# decision, rounded up (test_ilra_edge_cases_cpu.py recomputes every case's).  None does: the one flip of the table is at |t64| = 7.2e-8
# (cap_rowmap_act_8193, 2.1 M decisions), so every row-map case keeps the floor of 1e-6.  A longer or an fp32 case may not.
BANDS = {}
# name -> seed, where the enumeration's own had to be replaced to hold the yardstick: both draws went nearly one-hot, dE shrank to 1.5e-3
# and 5e-3 of its natural size and fp32 itself was 2.0e-5 and 3.7e-5 off
SEEDS = {"queries_pool_act_700_P1": 8104, "rising_pool_act_700_P5": 8102,
         # one query, rows sorted by it, E times 8: the enumeration's draws put 0.97 and 0.99 of the attention on the last row and dE at 5e-3 and
         # 5e-4 of its natural size.  fp32 on the CPU held them (5.1e-6, 3.3e-6), the kernels too (1.6e-5, 8.3e-5 -- 4e-8 of the natural
         # size), but a figure that is rounding noise against a cancelled sum says little; this draw leaves dE at a tenth of its natural size
         "rising_pool_bf16_700_P1": 8205, "rising_pool_f32_700_P1": 8205}

CASES = []


def _add(group, kind, sizes, src, P=8, stride=512, gain=1.0, order="random", xgrad=True, label=None):
    sizes = tuple(int(n) for n in sizes)
    name = f"{group}_{kind}_{src}_" + (label or "+".join(str(n) for n in sizes)) + (f"_P{P}" if kind == "pool" else "")
    assert name not in {c.name for c in CASES}, name
    band = None if kind == "pool" else BANDS.get(name, IC.BAND)
    CASES.append(EdgeCase(name, group, kind, sizes, src, P if kind == "pool" else 0, stride, gain, order, band,
                          bool(xgrad and src == "act"), SEEDS.get(name, 7000 + 13 * len(CASES))))


# The yardstick figures are the worst of a group over Z / xhat and every gradient, fp32 torch on the CPU against float64 by
# ilra_helpers.rel (gate: a quarter of TOL = 2.5e-5); measured by test_ilra_edge_cases_cpu.py, which prints each.  The largest are
# packed rows at N >= 700 (score spreads of 54 .. 72 and, with E times 4, of 200 .. 298): queries_pool_act_700_P16 1.7e-5,
# rising_pool_act_700_P16 1.7e-5, cap_pool_act_16384_P8 1.4e-5, all on dE.
# ---- packed rows without a gradient: k_ip_backward<float, 256, false>, k_rm_backward<float, 256, false> ---- yardstick 4.8e-6
for kind in ("pool", "rowmap"):
    _add("nograd", kind, (17, 33), "act", xgrad=False)
# ---- a row stride of 1024 under every kernel that reads src.ldx ---------------------------------------------- yardstick 1.6e-6
for src in ("bf16", "f32"):
    for N in (17, 300):
        for kind in ("pool", "rowmap"):
            _add("strided", kind, (N,), src, stride=1024)
# ---- ragged tables for every source: the bag lookup past bag 0, row offsets, a second b~ row, wgrad splits across bags --- yardstick 3.6e-6
# f32: 19 row-map tiles in 5 splits, split 0 walks the tiles 0, 5, 10, 15 = bags 0, 1, 3, 3
RAGGED = {"bf16": (33, 1, 300), "f32": (17, 130, 1, 300, 64), "act": (40, 257, 7, 33)}
for src, sizes in RAGGED.items():
    for kind in ("pool", "rowmap"):
        _add("ragged", kind, sizes, src)
# ---- every query count whose last register group is empty, partly or wholly valid ------------------------------- yardstick 1.7e-5
for P in (1, 4, 5, 15, 16):
    for src in ("bf16", "f32", "act"):
        for N in (1, 17, 700):
            _add("queries", "pool", (N,), src, P=P)
# ---- both sides of the two caps, and a capped bag followed by others -------------------------------------------- yardstick 1.4e-5
for src in ("bf16", "act"):
    for N in (16384, 16385):
        _add("cap", "pool", (N,), src)
    for N in (8192, 8193):
        _add("cap", "rowmap", (N,), src)
_add("cap", "pool", (16385, 1, 300), "bf16")
# ---- peaks: a maximum that rises on every tile (three parts), at the gains and P the yardstick admits ------------- yardstick 1.7e-5
for src in ("bf16", "f32"):
    for P in (1, 5, 16):
        _add("rising", "pool", (700,), src, P=P, gain=8.0, order="rising")
for P in (5, 16):
    _add("rising", "pool", (700,), "act", P=P, gain=4.0, order="rising")
# ---- peaks: one row ahead of every other by 120: parts that merge with weight 0 (N = 700), one part (N = 17: two tiles, N = 33:
# three, the last holds the one row) ------------------------------------------------------------------------------- yardstick 4.7e-6
for src in ("bf16", "f32", "act"):
    for N in (700, 33, 17):
        _add("spike", "pool", (N,), src, P=5, order="spike")
# ---- short bags: column-sum segments that are empty or hold one row ----------------------------------------------- yardstick 5.2e-7
for src in ("bf16", "f32", "act"):
    for N in (2, 7, 8, 9):
        _add("short", "rowmap", (N,), src)
# ---- the chunk limit: 64 bags of 1 .. 40 rows, the [64, 256] b~ gradient, dE over the parts of 64 bags ------------- yardstick 6.3e-6
CHUNK64 = tuple(1 + (7 * i) % 40 for i in range(64))
for src in ("bf16", "act"):
    for kind in ("pool", "rowmap"):
        _add("chunk", kind, CHUNK64, src, label="64bags")

BY_NAME = {c.name: c for c in CASES}


def names(group=None, kind=None):
    return [c.name for c in CASES if (group is None or c.group == group) and (kind is None or c.kind == kind)]


def width(case):
    return 256 if case.src == "act" else 512


def _to_bf16_values(x):
    return torch.from_numpy(np.ascontiguousarray(x)).bfloat16().float().numpy()


def make_inputs(case):
    """host-side inputs of a case: ``xs`` the bags' own rows (fp32 arrays [N_b, 512]; exact in bf16 unless src is "f32"), ``a`` the
    packed fp32 rows [sum N_b, 256] or None, ``rows`` what the kernels read as rows, per bag ([N_b, D] fp32); for the pooling ``E``
    [P, D] and ``G`` [B, P, D]; for the row map ``params`` (ilra_helpers.rowmap_params, one b~ row per bag) and ``G`` [sum N_b, 256]"""
    import ilra_helpers as IH
    rs = np.random.RandomState(case.seed)
    D, B, total = width(case), len(case.sizes), sum(case.sizes)
    kind = "f32" if case.src == "f32" else "bf16"
    xs = [IC.make_bag(n, kind, case.seed + 100 + i) for i, n in enumerate(case.sizes)]
    a = None
    if case.src == "act":
        a = (np.random.RandomState(case.seed + 7).standard_normal((total, 256)) * 0.4).astype(np.float32)
    out = {"xs": xs, "a": a}
    if case.kind == "pool":
        E = (rs.standard_normal((case.P, D)) * (0.5 if D == 512 else 1.5) * case.gain).astype(np.float32)
        out["E"], out["G"] = E, rs.standard_normal((B, case.P, D)).astype(np.float32)
        if case.order != "random":
            assert B == 1, "the score profiles are built for one bag"
            x = a if a is not None else xs[0]
            if case.order == "rising":
                x = x[np.argsort(x.astype(np.float64) @ E[0].astype(np.float64), kind="stable")]
            else:
                e = E[SPIKE_Q].astype(np.float64)
                s = x.astype(np.float64) @ e
                lift = SPIKE_MARGIN + float(s[:-1].max() if len(s) > 1 else 0.0) - float(s[-1])
                x = x.copy()
                x[-1] = (x[-1].astype(np.float64) + lift * e / float(e @ e)).astype(np.float32)
                if case.src == "bf16":
                    x[-1] = _to_bf16_values(x[-1])
            x = np.ascontiguousarray(x)
            if a is not None:
                out["a"] = a = x
            else:
                out["xs"] = xs = [x]
    else:
        out["params"] = IH.rowmap_params(rs, D, B)
        out["G"] = rs.standard_normal((total, 256)).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(case.sizes)])
    out["rows"] = xs if a is None else [a[offs[i]:offs[i + 1]] for i in range(B)]
    return out
