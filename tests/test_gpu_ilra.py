"""ILRA on the GPU.  The pooling and the row map alone against float64 (every row source, N around the tile heights and over several
parts: Z, xhat, dE, dX and the six row-map gradients); the module against the reference's float64 fixtures and the float64 restatement
evaluated with the KERNEL's ReLU decisions (logits, intermediates, every parameter gradient); the mask band; batches, chunks, the
``BagSet`` route, a strided bag, reproducibility, modes and refusals.  Every comparison prints its figure before it asserts.

The parity cases are "live" (ilra_cases.py): with the default initialisation every attention is uniform and a kernel that reads the
wrong rows would pass."""
import numpy as np
import pytest
import torch

import ilra_cases as IC
import ilra_helpers as IH

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = IH.TOL


def _bag(x, rows):
    return IH.bag(x, rows, DEV)


_rel = IH.rel          # within TOL of the largest float64 entry, with the ``natural`` rule (ilra_helpers.py)


# ---- the entry points alone --------------------------------------------------------------------------------------------------------
SIZES = [1, 15, 16, 17, 31, 32, 33, 700]          # the pooling's tile is 16 rows, the row map's 32; 700 rows = three pooling parts
SOURCES = [("bf16", 512), ("f32", 512), ("act", 256)]


def _source(N, src, seed):
    return IH.source(N, src, seed, DEV)


@pytest.mark.parametrize("src,D", SOURCES)
@pytest.mark.parametrize("N", SIZES)
def test_pooling_alone(N, src, D):
    from vlsa_amd import functional as VF
    rs = np.random.RandomState(400 + N)
    bags, xp, X = _source(N, src, 300 + N)
    E = torch.from_numpy((rs.standard_normal((8, D)) * (0.5 if D == 512 else 1.5)).astype(np.float32))
    G = torch.from_numpy(rs.standard_normal((1, 8, D)).astype(np.float32))
    Ed, Xd = E.double().requires_grad_(True), X.clone().requires_grad_(True)
    Z64 = torch.softmax(Xd @ Ed.t(), dim=0).t() @ Xd
    dE64, dX64 = torch.autograd.grad((Z64 * G[0].double()).sum(), [Ed, Xd])
    peak = float(torch.softmax(X @ E.double().t(), dim=0).max()) * N
    print(f"[ilra pool N={N} {src}] attention peak {peak:.1f} x uniform")
    Eg = E.to(DEV).requires_grad_(True)
    if xp is not None:
        xp.requires_grad_(True)
    Z = VF.ilra_pool_bags(bags, Eg, xp)
    (Z * G.to(DEV)).sum().backward()
    _rel(f"pool N={N} {src} Z", Z[0], Z64.detach().numpy())
    gx = float((X @ G[0].double().t()).abs().max())          # |g . x|: the size of a term of dE is |g . x| |x|, of dX |g|
    _rel(f"pool N={N} {src} dE", Eg.grad, dE64.numpy(), natural=gx * float(X.abs().max()))
    if xp is not None:
        _rel(f"pool N={N} {src} dX", xp.grad, dX64.numpy(), natural=float(G.abs().max()))


@pytest.mark.parametrize("src,D", SOURCES)
@pytest.mark.parametrize("N", SIZES)
def test_row_map_alone(N, src, D):
    from vlsa_amd import functional as VF
    rs = np.random.RandomState(500 + N)
    bags, xp, X = _source(N, src, 350 + N)
    names, P = IH.ROWMAP_KEYS, IH.rowmap_params(rs, D)
    G = torch.from_numpy(rs.standard_normal((N, 256)).astype(np.float32))
    Pg = {k: v.to(DEV).requires_grad_(True) for k, v in P.items()}
    if xp is not None:
        xp.requires_grad_(True)
    out, mask = VF.ilra_rowmap_bags(bags, Pg["Wq"], Pg["btil"], Pg["Wo"], Pg["bo"], Pg["Wg"], Pg["bg"], xp, ret_mask=True)
    (out * G.to(DEV)).sum().backward()
    bits = IH.unpack_mask(mask)
    Pd = {k: v.double().requires_grad_(True) for k, v in P.items()}
    Xd = X.clone().requires_grad_(True)
    u = Xd @ Pd["Wq"].t() + Pd["btil"]
    t = u @ Pd["Wo"].t() + Pd["bo"]
    IH.check_mask_band(f"rowmap N={N} {src}", bits.numpy(), t.detach().numpy())
    o64 = (u + t * bits.double()) * torch.nn.functional.silu(Xd @ Pd["Wg"].t() + Pd["bg"])
    g64 = torch.autograd.grad((o64 * G.double()).sum(), [Pd[k] for k in names] + [Xd])
    _rel(f"rowmap N={N} {src} xhat", out, o64.detach().numpy())
    for k, g in zip(names, g64):
        _rel(f"rowmap N={N} {src} d{k}", Pg[k].grad, g.numpy())
    if xp is not None:
        _rel(f"rowmap N={N} {src} dX", xp.grad, g64[-1].numpy())


# ---- the module --------------------------------------------------------------------------------------------------------------------
def _run(m, bags, w):
    """forward_bags with state, backward of sum(logits * w): logits, per-chunk states, gradients by key"""
    m.zero_grad(set_to_none=True)
    logits, states = m.forward_bags(bags, ret_state=True)
    (logits * torch.as_tensor(w, device=DEV)).sum().backward()
    return logits.detach(), states, {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _check_case(tag, m, x, rows, params, L, w, fx=None):
    logits, states, grads = _run(m, [_bag(x, rows)], w)
    st = states[0]
    masks = [IH.unpack_mask(st[f"mask{i}"]).numpy() for i in range(L)]
    l64, inter, _ = IH.run64(x, params, L, w)
    lscale = max(1.0, float(np.abs(l64).max()))
    el = float(np.abs(logits.double().cpu().numpy() - l64).max())
    print(f"[ilra {tag}] logits err {el:.2e} (gate {TOL * lscale:.1e}, max|logit| {float(np.abs(l64).max()):.3f})")
    assert el <= TOL * lscale, (tag, el)
    for i in range(L):
        _rel(f"{tag} Z{i}", st[f"Z{i}"][0], inter[f"Z{i}"])
        _rel(f"{tag} H{i}", st[f"H{i}"][0], inter[f"H{i}"])
        _rel(f"{tag} xhat{i}", st[f"xhat{i}"], inter[f"xhat{i}"])
        IH.check_mask_band(f"{tag} block {i}", masks[i], inter[f"t{i}"])
    _rel(f"{tag} Zp", st["Zp"][0], inter["Zp"])
    _, _, gk = IH.run64(x, params, L, w, masks=masks)
    IH.check_grads(tag + " vs the restatement with the kernel's masks", grads, gk)
    if fx is not None:
        ef = float(np.abs(logits.double().cpu().numpy() - fx["logits"]).max())
        print(f"[ilra {tag}] logits vs the reference's float64 fixture {ef:.2e}; dropping the last row moves them by "
              f"{float(fx['sens/drop_last']) if 'sens/drop_last' in fx else float('nan'):.1e} (relative)")
        assert ef <= TOL * lscale
        for i in range(L):
            _rel(f"{tag} Z{i} vs fixture", st[f"Z{i}"][0], fx[f"Z{i}"])
            _rel(f"{tag} H{i} vs fixture", st[f"H{i}"][0], fx[f"H{i}"])
        _rel(f"{tag} Zp vs fixture", st["Zp"][0], fx["Zp"])
        if all(np.array_equal(masks[i], inter[f"t{i}"] > 0) for i in range(L)):
            IH.check_digests(tag + " digests vs fixture", {k: g.double().cpu().numpy() for k, g in grads.items()}, fx,
                             IC.CASES[tag][4], TOL)


@pytest.mark.parametrize("name", IC.PARITY)
def test_fixture_case(name):
    N, rows, L, C, seed, _ = IC.CASES[name]
    x, params, w = IC.make_case(name)
    _check_case(name, IH.build_model(L, C, params, DEV), x, rows, params, L, w, IH.load_fixture(name))


def test_default_initialisation_loads_and_runs():
    """kept as a state-dict check only: this model cannot tell one bag from another"""
    N, rows, L, C, seed, _ = IC.CASES["default_n130"]
    x, params, w = IC.make_case("default_n130")
    m = IH.build_model(L, C, params, DEV)
    out = m(_bag(x, rows)[None])
    assert tuple(out.shape) == (1, C) and float(np.abs(out.detach().double().cpu().numpy() - IH.load_fixture("default_n130")["logits"]).max()) <= TOL


BATCH = [1, 17, 130, 2798, 64]


@pytest.fixture(scope="module")
def batch():
    params = IC.make_params(2, 4, 700)
    m = IH.build_model(2, 4, params, DEV)
    bags = [_bag(IC.make_bag(n, "bf16", 710 + i), "bf16") for i, n in enumerate(BATCH)]
    w = np.random.RandomState(72).standard_normal((len(BATCH), 4)).astype(np.float32)
    return m, bags, w


def test_batch_equals_single_calls_and_is_reproducible(batch):
    m, bags, w = batch
    logits, _, grads = _run(m, bags, w)
    singles, gsum = [], None
    for i, x in enumerate(bags):
        m.zero_grad(set_to_none=True)
        out = m(x[None])
        (out * torch.as_tensor(w[i:i + 1], device=DEV)).sum().backward()
        singles.append(out.detach())
        g = {k: p.grad.detach().double() for k, p in m.named_parameters()}
        gsum = g if gsum is None else {k: gsum[k] + g[k] for k in g}
    assert torch.equal(logits, torch.cat(singles)), float((logits - torch.cat(singles)).abs().max())
    IH.check_grads("batch vs the sum of single calls", grads, {k: g.cpu().numpy() for k, g in gsum.items()})
    again = _run(m, bags, w)
    assert torch.equal(again[0], logits) and all(torch.equal(again[2][k], grads[k]) for k in grads)


def test_bagset_route_strided_bag_and_two_chunks(batch):
    from vlsa_amd.functional import BagSet
    m, bags, w = batch
    with torch.no_grad():
        base = m.forward_bags(bags)
        assert torch.equal(m.forward_bags(BagSet(bags)), base)
        arena = torch.zeros(130, 1024, dtype=torch.bfloat16, device=DEV)
        arena[:, :512] = bags[2]
        view = arena[:, :512]
        assert view.stride(0) == 1024 and torch.equal(m.forward_bags([view]), base[2:3])
        many = [_bag(IC.make_bag(1 + (7 * i) % 40, "bf16", 800 + i), "bf16") for i in range(65)]
        out = m.forward_bags(many)
        assert tuple(out.shape) == (65, 4)
        assert torch.equal(out, torch.cat([m.forward_bags(many[:64]), m.forward_bags(many[64:])]))
        assert torch.equal(out[3:4], m(many[3][None]))
    _, _, g_list = _run(m, bags, w)
    _, _, g_set = _run(m, BagSet(bags), w)
    assert all(torch.equal(g_list[k], g_set[k]) for k in g_list)


def test_row_budget_cuts_chunks(batch, monkeypatch):
    m, bags, w = batch
    with torch.no_grad():
        base = m.forward_bags(bags)
        monkeypatch.setattr(type(m), "ROW_BUDGET", 150)
        out, states = m.forward_bags(bags, ret_state=True)
    assert len(states) == 3 and torch.equal(out, base)          # [1, 17, 130] | [2798] (over the budget: alone) | [64]


def test_modes_agree_and_refusals(batch):
    from vlsa_amd import VlsaNativeError
    m, bags, w = batch
    with torch.no_grad():
        assert torch.equal(m.train()(bags[2][None]), m.eval()(bags[2][None]))
    with pytest.raises(VlsaNativeError):
        m(torch.randn(1, 40, 512, device=DEV, requires_grad=True))
    with pytest.raises(VlsaNativeError):
        m(torch.randn(1, 40, 512))
    with pytest.raises(VlsaNativeError):
        m.forward_bags([torch.randn(0, 512, device=DEV)])
    with pytest.raises(VlsaNativeError):
        m.forward_bags([bags[0], bags[1].float()])
