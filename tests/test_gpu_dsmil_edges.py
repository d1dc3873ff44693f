"""DSMIL's HIP kernels (csrc/dsmil.hip) where the fixtures of test_gpu_dsmil.py do not reach: every {fp32, bf16} x class padding {4, 8, 16}
instantiation, class counts at the padding edges (1, 2, 3, 8, 9, 13, 16), row counts around the 32 / 64-row tiles, the 512-row parts and
the 64-part cap, one ragged batch of all of these, equal instance scores (the lowest row wins: per-lane scan, 16-way merge of a part,
merge of the parts), more than 64 bags per call (two launch chains, two dropout seeds), strided row views and rows of norm 8 and 30.

Reference: dsmil_helpers.reference_formula in float64 on the CPU with torch autograd (collapsed_formula where dropout masks are
restated), on bags of dsmil_cases.make_rows, parameters of make_params, loss weights of make_w.  Gates (dsmil_helpers.check_outputs,
shared with test_gpu_dsmil.py): critical rows exact, logits 1e-4 absolute, attention 1e-4 of its largest entry, each gradient
max(1e-4, 3 x e32) of the tensor's largest float64 entry, e32 the error of the same formula in fp32 torch on the CPU.  Every bag
must keep its two largest float64 instance scores of each class at least 1e-5 apart (dsmil_helpers.MARGIN; the copies of a tie test
left out): a condition on the inputs, asserted, met by the choice of seeds.

Unit-norm rows go with b_classifier.q.weight x 8 (as test_gpu_dsmil.py's synthetic bags: the raw initialisation gives scores within
0.01 of each other, an attention that is uniform whatever the kernel does); the scaled rows of the feature-scale test take it as drawn."""
import functools

import numpy as np
import pytest
import torch

import dsmil_cases as DC
import dsmil_helpers as DH

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
Q_SCALE = 8.0


def _rows(N, kind, seed, scale=1.0):
    """[N, 512] fp32 numpy: make_rows times scale, rounded to bf16 AFTER the scaling for kind == "bf16" (the values the kernels read)"""
    x = DC.make_rows(N, "f32", seed) * np.float32(scale)
    return DC._bf16_round(x) if kind == "bf16" else x


@functools.lru_cache(maxsize=None)
def _params(C, seed, q_scale=Q_SCALE):
    p = DC.make_params(C, seed, False, q_scale)
    return [torch.from_numpy(p[k]) for k in DC.KEYS]


def _model(C, seed, q_scale=Q_SCALE, drop=0.25):
    return DH.build_model(C, seed, DEV, drop=drop, q_scale=q_scale)


def _dev(x, kind):
    return torch.from_numpy(x).to(DT[kind]).to(DEV)


def _w(C, seed):
    return DC.make_w(C, seed).astype(np.float64)


def _grads(m):
    return [p.grad.clone() for p in DH.module_params(m)]


def _forward_backward(m, X, w):
    """m(X[None]) with attention and critical rows, and the gradients of sum(logits * w)"""
    m.zero_grad(set_to_none=True)
    logits, attn, crit = m(X[None], ret_with_attn=True, ret_critical=True)
    (logits * torch.as_tensor(w, dtype=torch.float32, device=DEV)).sum().backward()
    return logits.detach(), attn, crit[0], _grads(m)


def _need_margin(tag, r):
    print(f"[dsmil {tag}] float64 score margin {r['margin']:.2e} (needs {DH.MARGIN:.0e}), fp32 argmax equal: {r['same32']}")
    assert r["margin"] >= DH.MARGIN, (tag, "the inputs leave the critical row open: pick another seed", r["margin"])


def _check_single(tag, C, kind, x, pseed, wseed, q_scale=Q_SCALE, crit=None, ignore=(), zero=()):
    """one bag through ``forward`` against the float64 formula; returns (logits, attention [1, N], critical rows) for further assertions.
    zero: gradients that are zero by construction of the bag; float64 leaves rounding noise there (asserted: below 1e-12 of the case's
    largest gradient entry), which is replaced by the exact zero, so that the rule for identically zero gradients applies."""
    r = DH.torch_case(torch.from_numpy(x), _params(C, pseed, q_scale), [_w(C, wseed)], crit=crit, ignore=ignore)
    _need_margin(tag, r)
    big = max(float(np.abs(g).max()) for g in r["grads"][0].values())
    for k in zero:
        assert float(np.abs(r["grads"][0][k]).max()) <= 1e-12 * big, (tag, k)
        r["grads"][0][k] = np.zeros_like(r["grads"][0][k])
    logits, attn, cr, grads = _forward_backward(_model(C, pseed, q_scale), _dev(x, kind), _w(C, wseed))
    assert tuple(logits.shape) == (1, C) and tuple(attn.shape) == (1, x.shape[0]) and tuple(cr.shape) == (C,)
    DH.check_outputs(tag, logits, attn, cr, grads, DH.case_ref(r))
    return logits, attn, cr


# ---- a. class counts at the padding edges, both row types ---------------------------------------------------------------------------------
SWEEP_A = [(C, kind, N) for C in (1, 2, 3, 8, 9, 13, 16) for kind in ("f32", "bf16") for N in (33, 1100)]
SEED_A = {c: 701 + i for i, c in enumerate(SWEEP_A)}


@pytest.mark.parametrize("C,kind,N", SWEEP_A)
def test_class_counts_at_the_padding_edges(C, kind, N):
    """C = 8 and 16 fill the padding (reduce16's lane-to-class map with 2 and 1 lanes per class, no zero-filled query row), 1..3 leave
    most of it zero, 9 and 13 are the fp32 / bf16 CP = 16 kernels part-filled; N = 33: one part, a one-row last tile; 1100: three parts"""
    seed = SEED_A[(C, kind, N)]
    _, attn, _ = _check_single(f"classes C={C} {kind} N={N}", C, kind, _rows(N, kind, seed), seed, seed)
    total = float(attn.double().sum())
    assert abs(total - 1.0) <= 1e-5, ("the mean over the classes divides by C, not by the padded count", C, total)


# ---- b. row counts at the tile, part and part-cap boundaries --------------------------------------------------------------------------------
CONFIGS = {"bf16_c4": (4, "bf16", 790), "f32_c13": (13, "f32", 791)}          # name -> (C, rows, parameter seed): 64- and 32-row score tiles
SMALL_N = (31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025)
LARGE_N = (32767, 32768, 32769, 32801)      # 64 parts (the cap from 32257 rows on) of 16-17 32-row tiles, 8-9 64-row tiles: uneven shares
SWEEP_B = [(cfg, N) for N in SMALL_N for cfg in CONFIGS] + [(cfg, N) for cfg in CONFIGS for N in LARGE_N]
SEED_B = {c: 729 + i for i, c in enumerate(SWEEP_B)}
_BATCH_SUMS = {}


def _batch_dlogits(cfg, N):
    """the row of the ragged batch's random dlogits that belongs to the bag (cfg, N)"""
    return np.random.RandomState(SEED_B[(cfg, N)] + 3000).standard_normal((1, CONFIGS[cfg][0]))


@functools.lru_cache(maxsize=None)
def _sweep_b_ref(cfg, N):
    """the float64 reference of one bag of sweep b, computed ONCE per session: for make_w (the single call) and, from the same forward,
    for the bag's row of the ragged batch's dlogits -- those gradients are only summed (float64 and fp32) per configuration"""
    C, kind, pseed = CONFIGS[cfg]
    seed = SEED_B[(cfg, N)]
    r = DH.torch_case(torch.from_numpy(_rows(N, kind, seed)), _params(C, pseed), [_w(C, seed), _batch_dlogits(cfg, N)])
    s = _BATCH_SUMS.setdefault(cfg, {"g64": None, "g32": None})
    for key, g in (("g64", r["grads"][1]), ("g32", r["grads32"][1])):
        s[key] = g if s[key] is None else DH.sum_grads([s[key], g])
    ref = DH.case_ref(r)
    return dict(ref=ref, margin=r["margin"], same32=r["same32"])


@pytest.mark.parametrize("cfg,N", SWEEP_B)
def test_row_counts_at_the_tile_part_and_cap_boundaries(cfg, N):
    C, kind, pseed = CONFIGS[cfg]
    tag = f"rows {cfg} N={N}"
    r = _sweep_b_ref(cfg, N)
    _need_margin(tag, r)
    logits, attn, cr, grads = _forward_backward(_model(C, pseed), _dev(_rows(N, kind, SEED_B[(cfg, N)]), kind), _w(C, SEED_B[(cfg, N)]))
    DH.check_outputs(tag, logits, attn, cr, grads, r["ref"])


# ---- c. all of sweep b's bags of one row type in one ragged batch ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_one_ragged_batch_of_all_boundary_sizes_equals_the_single_calls(cfg):
    from vlsa_amd import functional as VF
    C, kind, pseed = CONFIGS[cfg]
    sizes = list(SMALL_N) + list(LARGE_N)
    refs = [_sweep_b_ref(cfg, N) for N in sizes]
    for N, r in zip(sizes, refs):
        _need_margin(f"batch {cfg} N={N}", r)
    bags = [_dev(_rows(N, kind, SEED_B[(cfg, N)]), kind) for N in sizes]
    G = torch.from_numpy(np.concatenate([_batch_dlogits(cfg, N) for N in sizes])).float().to(DEV)
    m = _model(C, pseed)
    with torch.no_grad():
        singles = [m(x[None], ret_with_attn=True, ret_critical=True) for x in bags]
    for how, arg in (("list", bags), ("BagSet", VF.BagSet(bags))):
        m.zero_grad(set_to_none=True)
        logits, attn, crit = m.forward_bags(arg, ret_with_attn=True, ret_critical=True)
        assert tuple(logits.shape) == (len(bags), C) and tuple(crit.shape) == (len(bags), C)
        for i, (lg, a, cr) in enumerate(singles):
            assert torch.equal(lg[0], logits[i]) and torch.equal(a, attn[i]) and torch.equal(cr[0], crit[i]), (how, sizes[i])
            assert crit[i].tolist() == refs[i]["ref"]["crit"], (how, sizes[i])
        (logits * G).sum().backward()
        s = _BATCH_SUMS[cfg]
        DH.check_grads(f"batch {cfg} {how}", _grads(m), DH.grad_ref(s["g64"], s["g32"]))
    # the part table the plan derives on the device is the library's vlsa_dsmil_parts(N), cap included
    plan = VF.DsmilBagsPlan.of(VF.BagSet(bags))
    parts = [int(VF.nat.load().vlsa_dsmil_parts(N)) for N in sizes]
    assert parts == [min(64, -(-N // 512)) for N in sizes] and parts[-4:] == [64] * 4
    assert plan.part_start.tolist() == [0] + np.cumsum(parts).tolist() and plan.n_parts == sum(parts)


# ---- d. equal instance scores resolve to the lowest row -------------------------------------------------------------------------------------
TIE_N = 1100      # three parts (part g: score tiles g, g + 3, ...); 1100 = 17 x 64 + 12 = 34 x 32 + 12: the last tile is partial


def _tie_rows(where, T, R):
    """where the copies of the winning row go; T: rows per score tile (64 for C <= 4, else 32), R = T / 16: rows per 16-lane group
    (group s = 4 * wave + grp of a tile holds its rows s * R .. s * R + R - 1; one lane scans its group's rows of all tiles of the part)"""
    return {
        "one_group": (T, T + 1),                           # tile 1, group 0: the per-lane scan keeps the first of equals
        "one_lane_two_tiles": (T, 4 * T + 1),              # tiles 1 and 4 (both part 1), group 0 in each: the same scan, a tile apart
        "two_waves": (T + 1, T + 8 * R + 1),               # tile 1, wave 0 and wave 2: the 16-way merge
        "two_tiles_of_a_part": (2 * T - 1, 4 * T),         # tile 1's LAST group and tile 4's FIRST: the merge meets the higher row first
        "two_parts": (T + 5, 3 * T + 2),                   # tile 1 (part 1) and tile 3 (part 0): the lower row is in the higher part
        "first_and_last_row": (0, TIE_N - 1),              # the rows past N - 1 of the last tile repeat row N - 1 and must never win
        "three_parts": (T + 5, 2 * T + 3, 3 * T + 2),      # parts 1, 2, 0
    }[where]


TIES = [(C, kind, where) for C in (4, 6) for kind in ("f32", "bf16")
        for where in ("one_group", "one_lane_two_tiles", "two_waves", "two_tiles_of_a_part", "two_parts", "first_and_last_row", "three_parts")]
SEED_T = {c: 820 + i for i, c in enumerate(TIES)}


@pytest.mark.parametrize("C,kind,where", TIES)
def test_equal_scores_resolve_to_the_lowest_row(C, kind, where):
    seed = SEED_T[(C, kind, where)]
    k = seed % C                                                    # the class whose winning row is duplicated
    T = 64 if C <= 4 else 32
    pos = _tie_rows(where, T, T // 16)
    lo = min(pos)
    P = _params(C, seed)
    x = _rows(TIE_N, kind, seed)
    scores = lambda a: torch.from_numpy(a).double() @ P[0].double().t()
    best = int(scores(x)[:, k].argmax())
    x[[best, lo]] = x[[lo, best]]                                   # the winner of class k to the lowest position ...
    before = scores(x).argmax(dim=0).tolist()
    assert before[k] == lo
    others = [p for p in pos if p != lo]
    assert not (set(before) & set(others)), "a copy would overwrite another class's critical row: pick another seed"
    x[others] = x[lo]                                               # ... and bit-for-bit copies of it to the others
    masked = scores(x)
    masked[others] = -float("inf")
    expect = masked.argmax(dim=0).tolist()
    assert expect == before                                         # the copies change no class's critical row
    tag = f"tie C={C} {kind} {where} k={k} rows={pos}"
    _, _, cr = _check_single(tag, C, kind, x, seed, seed, crit=expect, ignore=others)
    assert cr[k].item() == lo


@pytest.mark.parametrize("C,kind", [(4, "f32"), (4, "bf16"), (6, "f32"), (6, "bf16")])
def test_a_bag_of_identical_rows(C, kind):
    """N = 100 copies of one row: every class resolves to row 0 and the attention is uniform.  The weighted sum z equals every row,
    so ds[n, j] = A[n, j] (x_n . dz_j - z_j . dz_j) = 0: no gradient reaches b_classifier.q.* through the softmax"""
    N, seed = 100, 860 + C + (kind == "bf16")
    x = np.repeat(_rows(1, kind, seed), N, axis=0)
    _, attn, cr = _check_single(f"identical rows C={C} {kind}", C, kind, x, seed, seed, crit=[0] * C, ignore=range(1, N),
                                zero=("b_classifier.q.weight", "b_classifier.q.bias"))
    assert cr.tolist() == [0] * C
    assert float((attn - 1.0 / N).abs().max()) <= 1e-4 / N


# ---- e. more than 64 bags: two launch chains per call ---------------------------------------------------------------------------------------
MANY = {"bf16_c4": (4, "bf16", 792), "f32_c9": (9, "f32", 793)}


def _many_bags(kind):
    sizes = np.random.RandomState(870).randint(1, 701, size=70).tolist()
    sizes[3], sizes[40], sizes[66], sizes[69] = 1, 700, 1, 513          # the extremes, in both chunks
    return [_rows(n, kind, 900 + i) for i, n in enumerate(sizes)]


@pytest.mark.parametrize("cfg", list(MANY))
def test_seventy_bags_in_eval_mode_equal_the_per_bag_calls_and_two_explicit_calls(cfg):
    from vlsa_amd import functional as VF
    C, kind, pseed = MANY[cfg]
    xs = _many_bags(kind)
    bags = [_dev(x, kind) for x in xs]
    m = _model(C, pseed)
    G = torch.randn(70, C, generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        singles = [m(x[None], ret_with_attn=True, ret_critical=True) for x in bags]
    m.zero_grad(set_to_none=True)
    (m.forward_bags(bags[:64]) * G[:64]).sum().backward()
    (m.forward_bags(bags[64:]) * G[64:]).sum().backward()            # accumulates: the sum of the two explicit calls
    two = _grads(m)
    for how, arg in (("list", bags), ("BagSet", VF.BagSet(bags))):
        m.zero_grad(set_to_none=True)
        logits, attn, crit = m.forward_bags(arg, ret_with_attn=True, ret_critical=True)
        assert tuple(logits.shape) == (70, C) and tuple(crit.shape) == (70, C) and crit.dtype == torch.int32
        assert len(attn) == 70 and [tuple(a.shape) for a in attn] == [(1, x.shape[0]) for x in xs]
        for i, (lg, a, cr) in enumerate(singles):
            assert torch.equal(lg[0], logits[i]) and torch.equal(a, attn[i]) and torch.equal(cr[0], crit[i]), (how, i)
        (logits * G).sum().backward()
        for key, g, t in zip(DC.KEYS, _grads(m), two):
            e = float((g - t).abs().max() / t.abs().max())
            print(f"[dsmil 70 bags {cfg} {how}] d{key}: rel diff to the two explicit calls {e:.2e}, gate 1.00e-04")
            assert e <= 1e-4, (how, key, e)           # (the floor of the gradient gate: both sides are the same kernels)


@pytest.mark.parametrize("cfg", list(MANY))
def test_seventy_bags_in_training_mode_draw_one_dropout_seed_per_chunk(cfg):
    """``_dropout_seed_word`` advances the module's device counter by one per launch chain and hands out its value: with the counter
    at s - 1, bags 0..63 are masked by keep_mask(s, b, ...) and bags 64..69 by keep_mask(s + 1, b - 64, ...) -- the bag index restarts
    with the chunk.  Restated masks, collapsed formula, float64."""
    from vlsa_amd import functional as VF
    C, kind, pseed = MANY[cfg]
    p, s = 0.25, 515001
    xs = _many_bags(kind)
    P = _params(C, pseed)
    G = np.random.RandomState(871).standard_normal((70, C))
    m = _model(C, pseed).train()
    m._drop_counter = torch.tensor([s - 1], dtype=torch.int64, device=DEV)
    logits = m.forward_bags(VF.BagSet([_dev(x, kind) for x in xs]))
    (logits * torch.from_numpy(G).float().to(DEV)).sum().backward()
    assert int(m._drop_counter.item()) == s + 1
    rs = []
    for b, x in enumerate(xs):
        mask = DH.keep_mask(s + b // 64, b % 64, x.shape[0], p)
        rs.append(DH.torch_case(torch.from_numpy(x), P, [G[b:b + 1]], formula=DH.collapsed_formula, mask=mask, p=p))
        assert rs[-1]["margin"] >= DH.MARGIN, (b, rs[-1]["margin"])
    ref = np.concatenate([r["logits"] for r in rs])
    e = float(np.abs(logits.detach().double().cpu().numpy() - ref).max())
    print(f"[dsmil 70 bags dropout {cfg}] logits err {e:.2e}")
    assert e <= 1e-4
    # with chunk 1's seed word reused for chunk 2 the last six logits are visibly different: the check can tell the seeds apart
    reused = np.concatenate([DH.torch_case(torch.from_numpy(xs[b]), P, [G[b:b + 1]], formula=DH.collapsed_formula,
                                           mask=DH.keep_mask(s, b - 64, xs[b].shape[0], p), p=p)["logits"] for b in (64, 65, 67, 68, 69)])
    assert float(np.abs(reused - ref[[64, 65, 67, 68, 69]]).max()) > 1e-3
    DH.check_grads(f"70 bags dropout {cfg}", _grads(m), DH.grad_ref(DH.sum_grads([r["grads"][0] for r in rs]), DH.sum_grads([r["grads32"][0] for r in rs])))


# ---- f. rows that are strided views -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_strided_row_views_equal_their_contiguous_copies_bit_for_bit(kind):
    """column slices [:, 64:576] of a [N, 640] matrix (row stride 640) and every second row of a [2N, 512] matrix (row stride 1024):
    ``_bag2d`` hands such views on as they are (unit inner stride, rows 16-byte aligned), so the kernels read them through the
    descriptor's row stride"""
    from vlsa_amd import functional as VF
    C, pseed = 6, 794
    g = torch.Generator().manual_seed(5)
    wide = torch.nn.functional.normalize(torch.randn(1100, 640, generator=g), dim=1).to(DT[kind]).to(DEV)
    tall = torch.from_numpy(_rows(2 * 700, kind, 880)).to(DT[kind]).to(DEV)
    views = [wide[:, 64:576], tall[::2], wide[:33, 64:576], tall[1::2][:513]]
    assert [v.stride(0) for v in views] == [640, 1024, 640, 1024]
    for v in views:
        kept = VF._bag2d(v[None])
        assert kept.data_ptr() == v.data_ptr() and kept.stride() == v.stride() and not v.is_contiguous()      # no copy: the view itself
    copies = [v.contiguous() for v in views]
    m = _model(C, pseed)
    G = torch.randn(len(views), C, generator=g).to(DEV)

    def run(bags):
        m.zero_grad(set_to_none=True)
        logits, attn, crit = m.forward_bags(bags, ret_with_attn=True, ret_critical=True)
        (logits * G).sum().backward()
        return [logits.detach(), crit] + list(attn) + _grads(m)
    want = run(copies)
    for how, arg in (("list", views), ("BagSet", VF.BagSet(views))):
        for i, (a, b) in enumerate(zip(run(arg), want)):
            assert torch.equal(a, b), (how, i)
    for i, (v, c) in enumerate(zip(views, copies)):                 # and bag by bag through ``forward``
        a = _forward_backward(m, v, G[i:i + 1].cpu().numpy())
        b = _forward_backward(m, c, G[i:i + 1].cpu().numpy())
        for s, t in zip(list(a[:3]) + a[3], list(b[:3]) + b[3]):
            assert torch.equal(s, t), i
    # the copies are right (so the views are): the first against float64
    x = copies[1].float().cpu().numpy()
    r = DH.torch_case(torch.from_numpy(x), _params(C, pseed), [G[1:2].double().cpu().numpy()])
    _need_margin(f"strided {kind}", r)
    DH.check_outputs(f"strided {kind}", *_forward_backward(m, views[1], G[1:2].cpu().numpy()), DH.case_ref(r))


# ---- g. rows that are not unit-norm -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,kind,scale", [(C, kind, s) for C, kind in ((4, "f32"), (12, "bf16")) for s in (8.0, 30.0)])
def test_rows_of_norm_8_and_30(C, kind, scale):
    """un-normalised encoders: the softmax scores grow with the square of the norm (x 64, x 900: parameters as drawn, q_scale 1), the
    attention is near one-hot and the running-maximum rescale of the online softmax carries the result"""
    seed = 890 + int(scale) + C
    _check_single(f"norm {scale:g} C={C} {kind}", C, kind, _rows(2000, kind, seed, scale), seed, seed, q_scale=1.0)
