"""The ILRA edge-case table (ilra_edge_cases.py) without a GPU.  Placement: every case sits on the side of the cap, the tile or the
segment boundary its group is named for, by the library's own host-side arithmetic.  Yardstick: the case's formula in plain fp32 torch on
the CPU stays within a quarter of ``ilra_helpers.TOL`` of float64 by the measure the GPU test applies -- a case that fp32 itself cannot
hold is the input's fault and is changed in the table, never in the gate.  Mask band: recomputed per row-map case by the rule
``ilra_cases.BAND`` was made by."""
import numpy as np
import pytest
import torch

import ilra_cases as IC
import ilra_edge_cases as EC
import ilra_helpers as IH

YARD = IH.TOL / 4
FP32_EXP_RANGE = 87.3          # ln(2^126): a score spread above it takes expf(s - m) through every normal fp32 exponent


@pytest.fixture(scope="module")
def lib():
    from vlsa_amd import build, _native
    build.build_native()
    return _native.load()


def _tiles(lib, sizes):
    t = lib.vlsa_ilra_tile_rows()
    return [(n + t - 1) // t for n in sizes]


def _splits(lib, sizes, D):
    """the split count the library sizes the weight-gradient workspace by"""
    total, nt, B = sum(sizes), sum(_tiles(lib, sizes)), len(sizes)
    words = lib.vlsa_ilra_rowmap_backward_workspace_bytes(total, nt, B, D) // 4 - total * 256 * 4 - B * 3 * 8 * 256
    assert words > 0 and words % (256 * D) == 0
    return words // (256 * D)


def _scores32(case, inp):
    """fp32 scores [N, P] of a one-bag pooling case, and the float64 ones"""
    x, E = inp["rows"][0], inp["E"]
    return (torch.from_numpy(x) @ torch.from_numpy(E).t()).numpy(), x.astype(np.float64) @ E.astype(np.float64).T


def test_the_table_holds_what_the_gpu_test_replays():
    by = lambda g, k=None: [EC.BY_NAME[n] for n in EC.names(g, k)]
    assert all(c.src == "act" and not c.xgrad and c.sizes == (17, 33) for c in by("nograd")) and {c.kind for c in by("nograd")} == {"pool", "rowmap"}
    assert {(c.kind, c.src, c.sizes[0]) for c in by("strided")} == {(k, s, n) for k in ("pool", "rowmap") for s in ("bf16", "f32") for n in (17, 300)}
    assert all(c.stride == 1024 for c in by("strided")) and all(c.stride == 512 for c in EC.CASES if c.group != "strided")
    assert {c.src for c in by("ragged")} == {"bf16", "f32", "act"} and all(3 <= len(c.sizes) <= 5 for c in by("ragged"))
    assert {(c.P, c.src, c.sizes[0]) for c in by("queries")} == {(p, s, n) for p in (1, 4, 5, 15, 16) for s in ("bf16", "f32", "act") for n in (1, 17, 700)}
    assert {(c.src, c.sizes) for c in by("cap", "pool")} == {(s, (n,)) for s in ("bf16", "act") for n in (16384, 16385)} | {("bf16", (16385, 1, 300))}
    assert {(c.src, c.sizes) for c in by("cap", "rowmap")} == {(s, (n,)) for s in ("bf16", "act") for n in (8192, 8193)}
    assert {(c.src, c.P, c.gain) for c in by("rising")} == {(s, p, 8.0) for s in ("bf16", "f32") for p in (1, 5, 16)} | {("act", 5, 4.0), ("act", 16, 4.0)}
    assert {(c.src, c.sizes[0]) for c in by("spike")} == {(s, n) for s in ("bf16", "f32", "act") for n in (700, 33, 17)} and all(c.P > 1 for c in by("spike"))
    assert {(c.src, c.sizes[0]) for c in by("short")} == {(s, n) for s in ("bf16", "f32", "act") for n in (2, 7, 8, 9)}
    assert {(c.kind, c.src) for c in by("chunk")} == {(k, s) for k in ("pool", "rowmap") for s in ("bf16", "act")}
    assert all(len(c.sizes) == 64 and (min(c.sizes), max(c.sizes)) == (1, 40) for c in by("chunk"))          # the most bags a chunk takes
    assert all(c.xgrad == (c.src == "act") for c in EC.CASES if c.group != "nograd")
    assert all((c.band is None) == (c.kind == "pool") and (c.band is None or IC.BAND <= c.band <= 1e-5) for c in EC.CASES)


def test_caps_sit_on_both_sides(lib):
    rows, cap = lib.vlsa_ilra_pool_part_rows(), lib.vlsa_ilra_pool_parts(1 << 62)
    assert (rows, cap) == (256, 64)
    for c in (EC.BY_NAME[n] for n in EC.names("cap", "pool")):
        N = c.sizes[0]
        raw, got = (N + rows - 1) // rows, lib.vlsa_ilra_pool_parts(N)
        assert (raw, got) == ((64, 64) if N == 16384 else (65, 64)), c.name          # unclamped at 16384, clamped at 16385
        tiles = (N + 15) // 16
        assert len(range(0, tiles, got)) == (16 if N == 16384 else 17)              # tiles the first part walks
        # the host's sum and the device-side clamp of IlraPlan agree on every bag's first part
        n = torch.tensor(c.sizes)
        dev = torch.cumsum(torch.clamp(torch.div(n + (rows - 1), rows, rounding_mode="floor"), 1, cap), 0).tolist()
        assert dev == np.cumsum([lib.vlsa_ilra_pool_parts(k) for k in c.sizes]).tolist()
    assert np.cumsum([lib.vlsa_ilra_pool_parts(k) for k in (16385, 1, 300)]).tolist() == [64, 65, 67]
    for c in (EC.BY_NAME[n] for n in EC.names("cap", "rowmap")):
        N, D = c.sizes[0], EC.width(c)
        nt, R = _tiles(lib, c.sizes)[0], _splits(lib, c.sizes, D)
        assert (nt, (nt + 3) // 4, R) == ((256, 64, 64) if N == 8192 else (257, 65, 64)), c.name
        assert len(range(0, nt, R)) == (4 if N == 8192 else 5)                      # tiles the first split walks


def test_small_tables_sit_where_the_table_says(lib):
    for c in EC.CASES:
        if c.group in ("queries", "rising", "spike") and c.sizes[0] == 700:
            assert lib.vlsa_ilra_pool_parts(700) == 3 and (700 + 15) // 16 == 44
        if c.group in ("nograd", "short") or (c.group in ("queries", "spike") and c.sizes[0] < 700):
            assert all(lib.vlsa_ilra_pool_parts(n) == 1 for n in c.sizes)
    # ragged fp32: a weight-gradient split whose tiles lie in more than one bag, and bags behind bag 0 at nonzero row offsets
    c = EC.BY_NAME[EC.names("ragged", "rowmap")[1]]
    assert c.src == "f32"
    tiles = _tiles(lib, c.sizes)
    owner = np.repeat(np.arange(len(tiles)), tiles)
    R = _splits(lib, c.sizes, 512)
    assert (sum(tiles), R) == (19, 5) and owner[0::R].tolist() == [0, 1, 3, 3]
    for c in (EC.BY_NAME[n] for n in EC.names("ragged")):
        assert sum(lib.vlsa_ilra_pool_parts(n) for n in c.sizes) >= len(c.sizes)
    assert [lib.vlsa_ilra_pool_parts(n) for n in EC.RAGGED["act"]] == [1, 2, 1, 1] and [lib.vlsa_ilra_pool_parts(n) for n in EC.RAGGED["bf16"]] == [1, 1, 2]
    # short bags: the column sums' eight row segments [N s / 8, N (s + 1) / 8)
    seg = lambda N: [N * (s + 1) // 8 - N * s // 8 for s in range(8)]
    assert sorted(set(seg(2))) == [0, 1] and sorted(set(seg(7))) == [0, 1] and set(seg(8)) == {1} and sorted(seg(9)) == [1] * 7 + [2]
    # spike, one part: N = 17 is two tiles, N = 33 three; the last holds the one row
    assert ((17 + 15) // 16, 17 % 16, (33 + 15) // 16, 33 % 16) == (2, 1, 3, 1)


@pytest.mark.parametrize("name", EC.names("rising"))
def test_rising_cases_raise_the_maximum_on_every_tile(name, lib):
    c = EC.BY_NAME[name]
    inp = EC.make_inputs(c)
    s32, s64 = _scores32(c, inp)
    N, G = c.sizes[0], lib.vlsa_ilra_pool_parts(c.sizes[0])
    assert np.all(np.diff(s64[:, 0]) >= 0) and int(np.argmax(s64[:, 0])) // 16 == (N - 1) // 16          # the maximum is in the last tile
    tmax = np.array([s32[16 * t:16 * t + 16, 0].max() for t in range((N + 15) // 16)])
    for g in range(G):
        assert np.all(np.diff(tmax[g::G]) > 0), (name, g)                           # every tile of every part lifts the running maximum
    spread = s64.max(0) - s64.min(0)
    print(f"[ilra {name}] score spread per query {spread.min():.0f} to {spread.max():.0f}")
    assert spread[0] > FP32_EXP_RANGE


@pytest.mark.parametrize("name", EC.names("spike"))
def test_spike_cases_underflow_the_parts_without_the_row(name, lib):
    c = EC.BY_NAME[name]
    inp = EC.make_inputs(c)
    s32, s64 = _scores32(c, inp)
    N, G, q = c.sizes[0], lib.vlsa_ilra_pool_parts(c.sizes[0]), EC.SPIKE_Q
    margin = float(s64[-1, q] - s64[:-1, q].max())
    print(f"[ilra {name}] query {q}: the last row leads by {margin:.1f}")
    assert margin > 110 and 1 < c.P
    tile = np.arange(N) // 16
    pm = np.array([s32[(tile % G) == g, q].max() for g in range(G)], dtype=np.float32)
    w = np.exp(pm - pm.max(), dtype=np.float32)
    assert int((w == 0).sum()) == (2 if N == 700 else 0) and G == (3 if N == 700 else 1), (name, w)
    if c.src == "bf16":
        x = torch.from_numpy(inp["rows"][0])
        assert torch.equal(x.bfloat16().float(), x)                                 # still exact in bf16


def _natural_pool(rows, G):
    gx = max(float(np.abs(x.astype(np.float64) @ G[b].astype(np.float64).T).max()) for b, x in enumerate(rows))
    return gx * max(float(np.abs(x).max()) for x in rows), float(np.abs(G).max())


@pytest.mark.parametrize("name", EC.names())
def test_yardstick_and_band(name):
    """fp32 torch on the CPU against float64, every quantity the GPU test compares, by its measure at a quarter of its gate"""
    c = EC.BY_NAME[name]
    inp = EC.make_inputs(c)
    worst = 0.0
    if c.kind == "pool":
        Z64, dE64, dX64 = IH.pool_ref(inp["rows"], inp["E"], inp["G"])
        Z32, dE32, dX32 = IH.pool_ref(inp["rows"], inp["E"], inp["G"], dtype=torch.float32)
        nE, nX = _natural_pool(inp["rows"], inp["G"])
        for b in range(len(c.sizes)):
            worst = max(worst, IH.rel(f"{name} fp32 Z[{b}]", Z32[b], Z64[b], gate=YARD))
        worst = max(worst, IH.rel(f"{name} fp32 dE", dE32, dE64, natural=nE, gate=YARD))
        if c.src == "act":
            worst = max(worst, IH.rel(f"{name} fp32 dX", dX32, dX64, natural=nX, gate=YARD))
    else:
        o32, t32, m32, g32, dX32 = IH.rowmap_ref(inp["rows"], inp["params"], inp["G"], dtype=torch.float32)
        o64, t64, _, g64, dX64 = IH.rowmap_ref(inp["rows"], inp["params"], inp["G"], bits=m32)
        flips = m32 != (t64 > 0)
        fmax = float(np.abs(t64[flips]).max()) if flips.any() else 0.0
        need = max(IC.BAND, 10 * fmax)
        print(f"[ilra {name}] fp32 flips {int(flips.sum())} decisions, largest |t64| among them {fmax:.2e}: band needed {need:.2e}, table {c.band:.2e}")
        assert c.band >= need, (name, need)
        worst = max(worst, IH.rel(f"{name} fp32 xhat", o32, o64, gate=YARD))
        for k in IH.ROWMAP_KEYS:
            worst = max(worst, IH.rel(f"{name} fp32 d{k}", g32[k], g64[k], gate=YARD))
        if c.src == "act":
            worst = max(worst, IH.rel(f"{name} fp32 dX", dX32, dX64, gate=YARD))
    print(f"[ilra yardstick] {c.group} {name} worst {worst:.2e}")
