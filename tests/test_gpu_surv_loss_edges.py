"""The survival loss kernels (vlsa_amd/csrc/surv_objectives.hip) on the incidence family, at every bin count and batch size their launches
branch on -- the DPP kernel k_surv_terms_rows16 up to 16 bins, the one-thread-per-sample kernel k_surv_terms for 17 .. 64, each as one block per 32 samples
(vlsa_surv_loss) and as one block walking the batch (vlsa_surv_objective) -- against the float64 truth of tests/surv_loss_cases.py.
The gates are 8 x what a plain fp32 evaluation of the same formulas reaches (tests/test_surv_loss_cases_cpu.py measures them); gradients
are held relative to the largest entry of the float64 gradient.  Every comparison prints its measured error next to the gate."""
import pytest
import torch

import surv_loss_cases as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _dev(*tensors):
    return tuple(x.to(DEV) for x in tensors)


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _objective(c):
    from vlsa_amd.losses import SurvObjective
    return SurvObjective(weight_ifmle=c.w_ifmle, weight_emd=c.w_emd, alpha=c.alpha, eps=C.EPS, p=c.p, raw_distance=c.raw)


# ---- 1. the objective route: vlsa_surv_objective up to 4096 samples, vlsa_surv_loss + torch mean above
@pytest.mark.parametrize("c", C.OBJECTIVE_CASES, ids=C.ids(C.OBJECTIVE_CASES))
def test_objective_against_float64(c):
    from vlsa_amd import VlsaNativeError
    i, want = C.case_inputs(c), C.case_truth(c)
    x, t, e = _dev(i.logits, i.t, i.e)
    ls_log = torch.tensor(C.LOG_LOGIT_SCALE, device=DEV)
    obj = _objective(c)
    xd = x.clone().requires_grad_(True)
    got = obj(xd, t, e, log_logit_scale=ls_log)
    got.backward()
    ev, eg = C.rel_value(got.detach().cpu(), want.objective), C.rel_grad(xd.grad.cpu(), want.grad)
    print(f"{c.name}: objective {got.item():.9g} truth {float(want.objective):.9g} rel {ev:.2e} (gate {C.VALUE_RTOL:g}); "
          f"gradient rel to max|truth| = {float(want.grad.abs().max()):.3e}: {eg:.2e} (gate {C.GRAD_RTOL:g})")
    assert got.shape == () and xd.grad.shape == (c.B, c.K)
    assert ev <= C.VALUE_RTOL and eg <= C.GRAD_RTOL
    # value_and_grad: the same launch outside autograd, the same bits (one block's reach: refused beyond it)
    if c.B <= C.ONE_BLOCK_MAX_B:
        v, g = obj.value_and_grad(x, t, e, log_logit_scale=ls_log)
        assert _same_bits(v, got) and _same_bits(g, xd.grad)
    else:
        with pytest.raises(VlsaNativeError):
            obj.value_and_grad(x, t, e, log_logit_scale=ls_log)
    # the exponentiated scale handed over instead of the raw parameter
    xe = x.clone().requires_grad_(True)
    got_e = obj(xe, torch.stack([t.float(), e], dim=1), cur_logit_scale=ls_log.exp())
    got_e.backward()
    dv, dg = C.rel_value(got_e.detach().cpu(), got.detach().cpu()), C.rel_grad(xe.grad.cpu(), xd.grad.cpu())
    print(f"{c.name}: exp(ls) route vs log route: value {dv:.2e} gradient {dg:.2e} (gate 2e-06)")
    assert dv <= 2e-6 and dg <= 2e-6


# ---- 2. the per-sample route: out_ifmle, out_emd and the unscaled gradient, from incidences
@pytest.mark.parametrize("K,B", C.ROW_SHAPES)
def test_per_sample_values_and_gradient_rows_against_float64(K, B):
    from vlsa_amd.losses import SurvEMD, SurvIFMLE
    inc, t, e = C.row_inputs(K, B)
    w = torch.randn(B, generator=torch.Generator().manual_seed(7100 + 100 * K + B))       # the upstream gradient of each sample's loss
    for which in ("ifmle", "emd"):
        values, rows = C.row_truth(K, B, which)
        xd = inc.to(DEV).requires_grad_(True)
        if which == "ifmle":
            got = SurvIFMLE(reduction="none")(xd, *_dev(t, e))
            assert got.shape == (B, 1)
        else:
            got = SurvEMD(reduction="none")(xd, *_dev(t, e), C.ROW_LOGIT_SCALE)
            assert got.shape == (B,)
        (got.reshape(-1) * w.to(DEV)).sum().backward()
        ev = C.rel_value_rows(got.detach().cpu(), values)
        eg = C.rel_grad_rows(xd.grad.cpu(), rows * w.double().view(B, 1))
        print(f"K={K} B={B} {which}: per-sample values {ev:.2e} (gate {C.ROW_VALUE_RTOL:g}); gradient rows, each rel to its own max: {eg:.2e} "
              f"(gate {C.GRAD_RTOL:g})")
        assert ev <= C.ROW_VALUE_RTOL and eg <= C.GRAD_RTOL


# ---- 3. a sample's result does not depend on its place in the batch (a wrong chunk, row or lane index would show)
@pytest.mark.parametrize("K", [16, 17, 64])
def test_a_sample_gives_the_same_bits_wherever_it_sits(K):
    from vlsa_amd.losses import SurvEMD, SurvIFMLE, SurvObjective
    big, other = C.case_inputs(C.GRID[[c.name for c in C.GRID].index(f"grid-k{K}-b130")]), C.make_inputs(33, K, 7300 + K, 2.0)
    s = 100                     # chunk 3, row / lane 4 of its chunk
    batches = {                 # name -> (logits, t, e, where the sample sits)
        "130": (big.logits, big.t, big.e, s),
        "alone": (big.logits[s:s + 1], big.t[s:s + 1], big.e[s:s + 1], 0),
        "first of 33": (torch.cat([big.logits[s:s + 1], other.logits[1:]]), torch.cat([big.t[s:s + 1], other.t[1:]]),
                        torch.cat([big.e[s:s + 1], other.e[1:]]), 0),
    }
    ls_log = torch.tensor(C.LOG_LOGIT_SCALE, device=DEV)
    seen = {}
    for name, (logits, t, e, at) in batches.items():
        B = logits.shape[0]
        x, td, ed = _dev(logits, t, e)
        _, g = SurvObjective().value_and_grad(x, td, ed, log_logit_scale=ls_log)
        inc = torch.softmax(logits, dim=-1)            # on the host: the same incidences whatever the batch
        rows = {}
        for which in ("ifmle", "emd"):
            xd = inc.to(DEV).requires_grad_(True)
            got = SurvIFMLE(reduction="none")(xd, td, ed) if which == "ifmle" else SurvEMD(reduction="none")(xd, td, ed, C.LOGIT_SCALE)
            got.sum().backward()
            rows[which] = (got.detach().reshape(-1)[at].cpu(), xd.grad[at].cpu())
        seen[name] = (B, g[at].cpu(), rows)
    _, g1, rows1 = seen["alone"]                           # (1 / B = 1: the objective's gradient row IS the sample's unscaled row)
    for name in ("130", "first of 33"):
        B, g, rows = seen[name]
        for which in ("ifmle", "emd"):
            assert _same_bits(rows[which][0], rows1[which][0]) and _same_bits(rows[which][1], rows1[which][1]), (name, which)
        # the objective route writes gscale * row with gscale = 1.f / (float)B, one rounding each: "the row times B" is not recoverable
        # bit for bit, the row scaled by the same fp32 1 / B is
        want = g1 * (torch.tensor(1.0) / torch.tensor(float(B)))
        print(f"K={K} sample {s} {name}: objective gradient row max|diff| {float((g - want).abs().max()):.2e}")
        assert _same_bits(g, want), name


# ---- 4. labels outside [0, K) are clamped by both kernels
@pytest.mark.parametrize("K", [12, 17])
def test_labels_out_of_range_are_clamped(K):
    from vlsa_amd.losses import SurvEMD, SurvIFMLE, SurvObjective
    i = C.make_inputs(33, K, 7400 + K, 2.0)
    low, high = torch.arange(33) % 3 == 0, torch.arange(33) % 3 == 1
    t_out = torch.where(low, torch.full_like(i.t, -3), torch.where(high, torch.full_like(i.t, K + 5), i.t))
    t_in = torch.where(low, torch.zeros_like(i.t), torch.where(high, torch.full_like(i.t, K - 1), i.t))
    assert int(t_out.min()) == -3 and int(t_out.max()) == K + 5 and 0 <= int(t_in.min()) and int(t_in.max()) == K - 1
    x, e = _dev(i.logits, i.e)
    ls_log = torch.tensor(C.LOG_LOGIT_SCALE, device=DEV)
    v_out, g_out = SurvObjective().value_and_grad(x, t_out.to(DEV), e, log_logit_scale=ls_log)
    v_in, g_in = SurvObjective().value_and_grad(x, t_in.to(DEV), e, log_logit_scale=ls_log)
    assert _same_bits(v_out, v_in) and _same_bits(g_out, g_in) and bool(torch.isfinite(g_in).all())
    inc = torch.softmax(x, dim=-1)
    for which in ("ifmle", "emd"):
        res = []
        for t in (t_out, t_in):
            xd = inc.clone().requires_grad_(True)
            got = SurvIFMLE(reduction="none")(xd, t.to(DEV), e) if which == "ifmle" else SurvEMD(reduction="none")(xd, t.to(DEV), e, C.LOGIT_SCALE)
            got.sum().backward()
            res.append((got.detach(), xd.grad))
        assert _same_bits(res[0][0], res[1][0]) and _same_bits(res[0][1], res[1][1]), which


# ---- 5. the two kernels on the same problem: 12 bins (rows16), and the same 12 bins zero-padded to 17 (k_surv_terms)
def test_rows16_and_the_per_thread_kernel_agree_on_a_padded_problem():
    from vlsa_amd.losses import SurvIFMLE
    i = C.make_inputs(33, 12, 7500, 2.0)
    inc12 = torch.softmax(i.logits, dim=-1)
    inc17 = torch.cat([inc12, torch.zeros(33, 5)], dim=1)
    t, e = _dev(i.t, i.e)
    out = []
    for inc in (inc12, inc17):
        xd = inc.to(DEV).requires_grad_(True)
        got = SurvIFMLE(reduction="none")(xd, t, e)
        got.sum().backward()
        out.append((got.detach().reshape(-1).cpu(), xd.grad.cpu()))
    (v12, g12), (v17, g17) = out
    bit_equal = _same_bits(v12, v17) and _same_bits(g12, g17[:, :12].contiguous())
    dv = float(((v12 - v17).abs() / v12.abs()).max())
    dg = C.rel_grad_rows(g17[:, :12], g12)
    print(f"K = 12 (rows16) vs zero-padded K = 17 (k_surv_terms): values {dv:.2e} gradient rows {dg:.2e} (gate 1e-06); bit-equal: {bit_equal}")
    assert dv <= 1e-6 and dg <= 1e-6
    assert bool((g17[:, 12:] == 0).all())           # the padding bins lie beyond every label


# ---- 6. the objective against the per-sample route
@pytest.mark.parametrize("K", [16, 17])
@pytest.mark.parametrize("B", [33, C.ONE_BLOCK_MAX_B])
def test_objective_is_the_mean_of_the_per_sample_route(K, B):
    from vlsa_amd.losses import SurvEMD, SurvIFMLE, SurvObjective
    i = C.make_inputs(B, K, 5000 + 100 * K + B, 2.0)            # (the GRID / BIG inputs of this shape)
    x, t, e = _dev(i.logits, i.t, i.e)
    v, g = SurvObjective().value_and_grad(x, t, e, log_logit_scale=torch.tensor(C.LOG_LOGIT_SCALE, device=DEV))
    xd = x.clone().requires_grad_(True)
    inc = torch.softmax(xd, dim=-1)
    rows = SurvIFMLE(reduction="none")(inc, t, e).reshape(-1) + SurvEMD(reduction="none")(inc, t, e, C.LOGIT_SCALE).reshape(-1)
    rows.sum().backward()
    ev = C.rel_value(v.cpu(), rows.detach().double().mean().cpu())
    eg = C.rel_grad(g.cpu().double() * B, xd.grad.cpu())
    print(f"K={K} B={B}: objective vs float64 mean of the per-sample values {ev:.2e} (gate {C.VALUE_RTOL:g}); B x gradient vs per-sample "
          f"gradient {eg:.2e} (gate {C.GRAD_RTOL:g})")
    assert ev <= C.VALUE_RTOL and eg <= C.GRAD_RTOL


# ---- 7. reproducibility and limits
@pytest.mark.parametrize("K", [17, C.MAX_K])
def test_two_calls_give_the_same_bits(K):
    from vlsa_amd.losses import SurvEMD, SurvIFMLE, SurvObjective
    i = C.make_inputs(130, K, 5000 + 100 * K + 130, 2.0)
    x, t, e = _dev(i.logits, i.t, i.e)
    ls_log = torch.tensor(C.LOG_LOGIT_SCALE, device=DEV)
    (v1, g1), (v2, g2) = (SurvObjective().value_and_grad(x, t, e, log_logit_scale=ls_log) for _ in range(2))
    assert _same_bits(v1, v2) and _same_bits(g1, g2)
    inc = torch.softmax(x, dim=-1)
    for module, extra in ((SurvIFMLE(reduction="none"), ()), (SurvEMD(reduction="none"), (C.LOGIT_SCALE,))):
        res = []
        for _ in range(2):
            xd = inc.clone().requires_grad_(True)
            got = module(xd, t, e, *extra)
            got.sum().backward()
            res.append((got.detach(), xd.grad))
        assert _same_bits(res[0][0], res[1][0]) and _same_bits(res[0][1], res[1][1])


def test_more_than_max_k_bins_are_refused_on_both_entry_points():
    from vlsa_amd import VlsaNativeError
    from vlsa_amd.losses import SurvEMD, SurvIFMLE, SurvObjective
    i = C.make_inputs(5, C.MAX_K + 1, 7700, 2.0)
    x, t, e = _dev(i.logits, i.t, i.e)
    ls_log = torch.tensor(C.LOG_LOGIT_SCALE, device=DEV)
    with pytest.raises(VlsaNativeError):
        SurvObjective()(x, t, e, log_logit_scale=ls_log)
    with pytest.raises(VlsaNativeError):
        SurvObjective().value_and_grad(x, t, e, log_logit_scale=ls_log)
    with pytest.raises(VlsaNativeError):
        SurvIFMLE(reduction="none")(torch.softmax(x, dim=-1), t, e)
    with pytest.raises(VlsaNativeError):
        SurvEMD()(torch.softmax(x, dim=-1), t, e, C.LOGIT_SCALE)
    served = SurvObjective()(x[:, :C.MAX_K].contiguous(), t, e, log_logit_scale=ls_log)        # 64 bins are served
    assert bool(torch.isfinite(served))
