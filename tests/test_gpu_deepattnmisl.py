"""DeepAttnMISL on the GPU against the reference's float64 fixtures and the float64 helper: logits and h_cluster to 1e-4, the ReLU mask
band (the kernel's decisions equal pre64 > 0 wherever |pre64| >= 1e-6, and the disagreeing set lies inside the stored near-zero list), all
twelve gradients to 1e-4 of the tensor's largest entry against the helper evaluated with the kernel's own mask (and against the stored
gradients where the masks agree), the tile and part boundaries, empty clusters, out-of-range ids, batches, reproducibility, modes and
refusals.

Every comparison prints its figure before it asserts.  The module's tail is evaluated in float64 (see the class docstring): the attention
branch's gradients are 1e-7 .. 1e-10 of the others in size and fp32 resolves them to about 2e-3 of their largest entry only."""
import numpy as np
import pytest
import torch

import deepattnmisl_cases as AC
import deepattnmisl_helpers as AH
from dsmil_cases import make_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bag(x, rows):
    t = torch.from_numpy(x).to(DEV)
    return (t.bfloat16() if rows == "bf16" else t).contiguous()


def _run(m, bags, idss, w):
    """forward_bags with state, backward of sum(logits * w): logits, hc, cnt, mask bits, gradients (AC.KEYS order)"""
    m.zero_grad(set_to_none=True)
    logits, hc, cnt, mask = m.forward_bags(bags, idss, ret_state=True)
    (logits * torch.as_tensor(w, device=DEV)).sum().backward()
    return logits.detach(), hc.detach(), cnt, AH.unpack_mask(mask), [p.grad.detach().clone() for p in AH.params_of(m)]


def _check_against_helper(tag, m, x, ids, Kc, w, rows, fx=None):
    """one bag: forward and backward against float64 (the helper; with fx also the reference's stored outputs)"""
    P = [p.detach().cpu() for p in AH.params_of(m)]
    logits, hc, cnt, bits, grads = _run(m, [_bag(x, rows)], [torch.from_numpy(ids).float()[None]], w)
    l64, h64, pre, g64 = AH.run64(x, ids, P, Kc, w)
    el, eh = float(np.abs(logits.double().cpu().numpy() - l64).max()), float(np.abs(hc[0].double().cpu().numpy() - h64).max())
    print(f"[deepattnmisl {tag}] logits err {el:.2e}, hc err {eh:.2e} (gate {AH.TOL:.0e})")
    assert el <= AH.TOL and eh <= AH.TOL, (tag, el, eh)
    assert cnt[0].cpu().tolist() == np.bincount(ids[(ids >= 0) & (ids < Kc)], minlength=Kc).tolist()
    same = AH.check_mask_band(tag, bits, pre, None if fx is None else (fx["near_row"], fx["near_unit"]))
    _, _, _, gk = AH.run64(x, ids, P, Kc, w, mask=bits)
    AH.check_grads(tag + " vs helper with the kernel's mask", grads, gk)
    if fx is not None:
        assert float(np.abs(logits.double().cpu().numpy() - fx["logits"]).max()) <= AH.TOL
        assert float(np.abs(hc[0].double().cpu().numpy() - fx["hc"]).max()) <= AH.TOL
        if same:
            AH.check_grads(tag + " vs the reference's stored gradients", grads, {k: fx["grad/" + k].astype(np.float64) for k in AC.KEYS})
    return same


@pytest.mark.parametrize("name", list(AC.CASES))
def test_fixture_case(name):
    N, Kc, num_cls, rows, seed = AC.CASES[name]
    x, ids, _, w = AC.make_case(name)
    m = AH.build_model(Kc, num_cls, seed, DEV)
    _check_against_helper(name, m, x, ids, Kc, w, rows, AH.load_fixture(name))


def _tile():
    from vlsa_amd import _native
    return int(_native.load().vlsa_cluster_pool_tile_rows())


@pytest.mark.parametrize("dn", [-1, 0, 1, 2])
@pytest.mark.parametrize("rows", ["bf16", "f32"])
def test_tile_and_part_boundaries(dn, rows):
    """N at the row tile - 1, at the tile, + 1 (the smallest N with two parts; the tile itself is that N - 1) and + 2"""
    N, Kc = _tile() + dn, 8
    x, ids = make_rows(N, rows, 50 + dn), AC.make_ids(N, Kc, 50 + dn)
    _check_against_helper(f"N={N} {rows}", AH.build_model(Kc, 2, 51, DEV), x, ids, Kc, AC.make_w(2, 51), rows)


@pytest.mark.parametrize("what", ["one_cluster", "two_empty", "out_of_range", "kc1", "kc16"])
def test_cluster_edges(what):
    N, Kc = 200, {"kc1": 1, "kc16": 16}.get(what, 8)
    x, ids = make_rows(N, "bf16", 60), AC.make_ids(N, Kc, 60)
    if what == "one_cluster":
        ids[:] = 3
    elif what == "two_empty":
        ids[(ids == 2) | (ids == 5)] = 0
    elif what == "out_of_range":
        ids[10:20], ids[100:120] = -1, Kc
    m = AH.build_model(Kc, 2, 61, DEV)
    _check_against_helper(what, m, x, ids, Kc, AC.make_w(2, 61), "bf16")
    if what == "two_empty":
        hc = m.cluster_features([_bag(x, "bf16")], [torch.from_numpy(ids)])
        assert bool((hc[0, [2, 5]] == 0).all())


def _max_parts():
    from vlsa_amd import _native
    return int(_native.load().vlsa_cluster_pool_parts(1 << 62))


@pytest.mark.parametrize("rows", ["bf16", "f32"])
@pytest.mark.parametrize("which", ["first_second_tile", "20000"])
def test_parts_that_own_several_tiles(which, rows):
    """beyond tile x max-parts rows a workgroup walks more than one tile: the running sums and counts carried from tile to tile, the
    staging buffers reused, the merge over parts of unequal tile counts.  The smallest such N (one part has two tiles, the second of
    one row) and 20 000 rows (313 tiles on 128 parts: two or three each)."""
    N, Kc = (_tile() * _max_parts() + 1 if which == "first_second_tile" else 20000), 8
    x, ids = make_rows(N, rows, 95), AC.make_ids(N, Kc, 95)
    ids[N - 1] = 5                       # the lone row of the last tile belongs to a cluster
    _check_against_helper(f"N={N} {rows}", AH.build_model(Kc, 2, 96, DEV), x, ids, Kc, AC.make_w(2, 96), rows)


def test_a_row_of_no_cluster_may_hold_anything_in_the_forward():
    """ids outside [0, Kc) keep a row out of every sum as an exact zero: Inf and NaN in such rows give the bits that zeros give"""
    N, Kc = 200, 8
    x, ids = make_rows(N, "f32", 97), AC.make_ids(N, Kc, 97)
    ids[[20, 21, 130]] = [-1, Kc, 1000]
    m = AH.build_model(Kc, 2, 98, DEV)
    for rows in ("bf16", "f32"):
        clean, dirty = x.copy(), x.copy()
        clean[[20, 21, 130]] = 0
        dirty[20], dirty[21, ::3], dirty[130, 5] = np.inf, np.nan, -np.inf
        with torch.no_grad():
            a = m.cluster_features([_bag(clean, rows)], [torch.from_numpy(ids)])
            b = m.cluster_features([_bag(dirty, rows)], [torch.from_numpy(ids)])
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b), rows


BATCH = [8, 2798, 17, 600, 257]


# 64 bags, the table's last lane in use: 1 + (7 i) % 40 rows each, bag 63 raised to 130 rows = three forward tiles and parts, five
# backward tiles
BATCH64 = [1 + (7 * i) % 40 for i in range(63)] + [130]


def _make_batch(sizes):
    m = AH.build_model(8, 4, 71, DEV)
    xs = [make_rows(n, "bf16", 80 + i) for i, n in enumerate(sizes)]
    idss = [AC.make_ids(max(n, 8), 8, 80 + i)[:n] for i, n in enumerate(sizes)]          # (a bag of fewer than 8 rows leaves clusters empty)
    w = np.random.RandomState(72).standard_normal((len(sizes), 4)).astype(np.float32)
    return m, [_bag(x, "bf16") for x in xs], [torch.from_numpy(i) for i in idss], w


@pytest.fixture(scope="module")
def batch():
    return _make_batch(BATCH)


def test_batch_equals_single_calls_and_is_reproducible(batch):
    for tag, (m, bags, idss, w) in (("batch", batch), ("64 bags", _make_batch(BATCH64))):
        _batch_equals_single_calls_and_is_reproducible(tag, m, bags, idss, w)


def _batch_equals_single_calls_and_is_reproducible(tag, m, bags, idss, w):
    logits, hc, _, _, grads = _run(m, bags, idss, w)
    singles, gsum = [], None
    for i, (x, c) in enumerate(zip(bags, idss)):
        m.zero_grad(set_to_none=True)
        out = m(x[None], c.float()[None])                      # [1, N] float ids as the reference's loader hands them
        (out * torch.as_tensor(w[i:i + 1], device=DEV)).sum().backward()
        singles.append(out.detach())
        g = [p.grad.detach().double() for p in AH.params_of(m)]
        gsum = g if gsum is None else [a + b for a, b in zip(gsum, g)]
    assert torch.equal(logits, torch.cat(singles)), (tag, float((logits - torch.cat(singles)).abs().max()))
    AH.check_grads(tag + " vs the sum of single calls", grads, {k: g.cpu().numpy() for k, g in zip(AC.KEYS, gsum)})
    again = _run(m, bags, idss, w)
    assert torch.equal(again[0], logits) and torch.equal(again[1], hc) and all(torch.equal(a, b) for a, b in zip(again[4], grads)), tag


def test_cpu_float_row_vector_ids_and_modes(batch):
    m, bags, idss, w = batch
    x, c = bags[3], idss[3]
    base = m(x[None], c)
    assert torch.equal(m(x, c.float()[None].cpu()), base) and torch.equal(m(x, c.to(DEV).int()), base) and tuple(base.shape) == (1, 4)
    m0 = AH.build_model(8, 4, 71, DEV, dropout=0.0)
    assert torch.equal(m0.train()(x[None], c), m0.eval()(x[None], c))
    mt = AH.build_model(8, 4, 71, DEV, dropout=0.25).train()
    mt(x[None], c).sum().backward()
    conv = mt.phis[0]
    assert bool(torch.isfinite(conv.weight.grad).all()) and bool(torch.isfinite(conv.bias.grad).all()) and float(conv.weight.grad.abs().max()) > 0


def test_refusals():
    from vlsa_amd import DeepAttnMISL, VlsaNativeError
    ids = torch.zeros(40)
    with pytest.raises(VlsaNativeError):
        AH.build_model(8, 1, 90, DEV)(torch.randn(1, 40, 512, device=DEV, requires_grad=True), ids)
    with pytest.raises(VlsaNativeError):
        DeepAttnMISL(dim_in=1024).to(DEV)(torch.randn(1, 40, 1024, device=DEV), ids)
    with pytest.raises(VlsaNativeError):
        DeepAttnMISL(num_clusters=17).to(DEV)(torch.randn(1, 40, 512, device=DEV), ids)
    with pytest.raises(VlsaNativeError):
        AH.build_model(8, 1, 90, DEV)(torch.randn(1, 40, 512), ids)
