"""The handler's other objectives on the device (vlsa_amd/csrc/surv_objectives.hip): the hazard family -- SurvMLE + SurvEMD behind the
sigmoid -- and SurvT2I, at every bin count and batch size the launches branch on, against the float64 restatement of
tests/objective_cases.py (which tests/test_objective_cases_cpu.py pins to the reference's own float64 results).  The gates are 8 x what a
plain fp32 evaluation of the same formulas reaches, measured there; every comparison prints its measured error next to the gate."""
import ctypes

import pytest
import torch

import cases
import objective_cases as C
import surv_loss_cases as S
import text_cases as TC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _dev(*tensors):
    return tuple(x.to(DEV) for x in tensors)


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _direct_objective(x, t, e, ls_log, alpha, eps, p, raw, w_ifmle, w_emd):
    """objective | gradient [1 + B K] of a direct call of vlsa_surv_objective on raw logits with the raw (log) logit scale"""
    from vlsa_amd import _native as nat
    B, K = x.shape
    out = torch.full((1 + B * K,), float("nan"), device=DEV)
    ptr = lambda v: ctypes.c_void_p(v.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert nat.load().vlsa_surv_objective(ptr(x), ptr(t), ptr(e), B, K, 1, ptr(ls_log), 1, alpha, eps, p, int(raw), w_ifmle, w_emd, ptr(out),
                                          ptr(out[1:]), stream) == 0
    return out


def _objective(family, alpha=0.0, p=2, raw=True, w=(1.0, 1.0, 0.5), t2i_loss="CL", t2i_reduction="mean"):
    from vlsa_amd.losses import SurvObjective
    hazard = family == "hazard"
    return SurvObjective(weight_ifmle=0.0 if hazard else w[0], weight_mle=w[0] if hazard else 0.0, weight_emd=w[1], alpha=alpha, eps=C.EPS, p=p,
                         raw_distance=raw, converter="sigmoid" if hazard else "softmax", weight_t2i=w[2], t2i_loss=t2i_loss,
                         t2i_reduction=t2i_reduction)


def _check_routes(name, family, obj, x, t, e, want, B):
    """value and gradient from forward().backward(), from (3 loss).backward() and from value_and_grad, with the raw and with the
    exponentiated logit scale, against the float64 truth `want`"""
    vg, gg = C.VALUE_RTOL[family], C.GRAD_RTOL[family]
    ls_log = torch.tensor(C.LOG_LOGIT_SCALE, device=DEV)
    xd = x.clone().requires_grad_(True)
    got = obj(xd, t, e, log_logit_scale=ls_log)
    got.backward()
    ev, eg = C.rel_value(got.detach().cpu(), want.objective), C.rel_grad(xd.grad.cpu(), want.grad, B)
    print(f"{name}: objective {got.item():.9g} truth {float(want.objective):.9g} rel {ev:.2e} (gate {vg:g}); gradient rel to "
          f"max(max|truth| = {float(want.grad.abs().max()):.3e}, 1/B): {eg:.2e} (gate {gg:g})")
    assert got.shape == () and xd.grad.shape == x.shape and bool(torch.isfinite(xd.grad).all())
    assert ev <= vg and eg <= gg
    x3 = x.clone().requires_grad_(True)
    (3.0 * obj(x3, t, e, log_logit_scale=ls_log)).backward()
    e3 = C.rel_grad(x3.grad.cpu(), 3.0 * want.grad, B / 3.0)
    print(f"{name}: gradient of 3 x loss {e3:.2e} (gate {gg:g})")
    assert e3 <= gg
    v, g = obj.value_and_grad(x, t, e, log_logit_scale=ls_log)         # the same launches outside autograd: the same bits
    if B <= C.ONE_BLOCK_MAX_B:
        assert _same_bits(v, got) and _same_bits(g, xd.grad)
    else:
        assert C.rel_value(v.cpu(), want.objective) <= vg and C.rel_grad(g.cpu(), want.grad, B) <= gg
    xe = x.clone().requires_grad_(True)                                 # the exponentiated scale handed over instead of the raw parameter
    got_e = obj(xe, torch.stack([t.float(), e], dim=1), cur_logit_scale=ls_log.exp())
    got_e.backward()
    dv, dg = C.rel_value(got_e.detach().cpu(), want.objective), C.rel_grad(xe.grad.cpu(), want.grad, B)
    print(f"{name}: exp(ls) route: value {dv:.2e} gradient {dg:.2e}")
    assert dv <= vg and dg <= gg
    return got, xd.grad


# ---- 1. the objective: vlsa_surv_objective_terms up to 4096 samples, vlsa_surv_terms + vlsa_surv_t2i + torch adds above
@pytest.mark.parametrize("c", C.OBJECTIVE_CASES, ids=C.ids(C.OBJECTIVE_CASES))
def test_objective_against_float64(c):
    i, want = C.case_inputs(c), C.case_truth(c)
    x, t, e = _dev(i.logits, i.t, i.e)
    obj = _objective(c.family, c.alpha, c.p, c.raw, (c.w_main, c.w_emd, c.w_t2i), c.t2i_loss, c.t2i_reduction)
    got, grad = _check_routes(c.name, c.family, obj, x, t, e, want, c.B)
    if c.family == "incidence" and c.w_t2i == 0 and c.B <= C.ONE_BLOCK_MAX_B:      # nothing new asked: the bits of vlsa_surv_objective
        out = _direct_objective(x, t, e, torch.tensor(C.LOG_LOGIT_SCALE, device=DEV), c.alpha, C.EPS, c.p, c.raw, c.w_main, c.w_emd)
        assert _same_bits(got, out[0]) and _same_bits(grad, out[1:].view(c.B, c.K))


@pytest.mark.parametrize("c", C.FIXTURES, ids=C.ids(C.FIXTURES))
def test_objective_against_the_references_float64_results(c):
    fx = C.load_fixture(c)
    x, t, e = _dev(torch.from_numpy(fx["logits"]), torch.from_numpy(fx["t"]), torch.from_numpy(fx["e"]))
    obj = _objective(c.family, c.alpha, c.p, c.raw, (c.w_main, c.w_emd, c.w_t2i), c.t2i_loss, c.t2i_reduction)
    xd = x.clone().requires_grad_(True)
    got = obj(xd, t, e, cur_logit_scale=torch.tensor(float(fx["logit_scale"]), device=DEV))
    got.backward()
    ev = C.rel_value(got.detach().cpu(), fx["ref64_total"])
    eg = C.rel_grad(xd.grad.cpu(), torch.from_numpy(fx["ref64_grad"]), c.B)
    print(f"{c.name}: value {ev:.2e} (gate {C.VALUE_RTOL[c.family]:g}) gradient {eg:.2e} (gate {C.GRAD_RTOL[c.family]:g})")
    assert ev <= C.VALUE_RTOL[c.family] and eg <= C.GRAD_RTOL[c.family]


# ---- 2. edges, each its own small case
@pytest.mark.parametrize("t2i_loss", ["CL", "KL"])
@pytest.mark.parametrize("K", C.EDGE_BINS)
@pytest.mark.parametrize("family,name", [(f, n) for f in C.FAMILIES for n in C.EDGE_NAMES[f]])
def test_edges_against_float64(family, name, K, t2i_loss):
    logits, t, e = C.EDGES[name](K)
    want = C.edge_truth(name, K, family, t2i_loss)
    x, td, ed = _dev(logits, t, e)
    obj = _objective(family, 0.3, 2, True, (1.0, 1.0, 0.5), t2i_loss, "mean")
    _, grad = _check_routes(f"{name}-{family}-k{K}-{t2i_loss}", family, obj, x, td, ed, want, logits.shape[0])
    # SurvT2I alone on the same inputs
    from vlsa_amd.losses import SurvT2I
    xd = x.clone().requires_grad_(True)
    v = SurvT2I(loss=t2i_loss)(xd, td, ed, C.LOGIT_SCALE)
    v.backward()
    w64 = C.truth(logits, t, e, C.LOGIT_SCALE, family, w_main=0.0, w_emd=0.0, w_t2i=1.0, t2i_loss=t2i_loss)
    assert C.rel_value(v.detach().cpu(), w64.t2i) <= C.VALUE_RTOL[family] and C.rel_grad(xd.grad.cpu(), w64.grad) <= C.GRAD_RTOL[family]
    if name in C.NO_COUNTED_BIN:            # a zero TENSOR with a zero gradient, no NaN
        assert isinstance(v, torch.Tensor) and v.item() == 0.0 and not bool(xd.grad.any())
    if name == "one-event":                 # log-softmax of one entry
        assert v.item() == 0.0 and not bool(xd.grad.any())
    if name == "censored-at-t0":            # takes part in no bin
        assert not bool(xd.grad[0].any()) and bool(xd.grad[1].any())
    if name == "bin-without-a-positive":    # bin 0: participants, no positive: skipped
        assert not bool(xd.grad[:, 0].any()) and bool(xd.grad[:, 1].any())
    if family == "hazard" and name == "h-below-eps":
        # the event's -log clamp(h_t) passes no gradient: what is left at (0, t) is S_padded's share (none: bin t is not below t), SurvEMD's and SurvT2I's
        w_mle = C.truth(logits, t, e, C.LOGIT_SCALE, family, 0.3, w_main=1.0, w_emd=0.0).grad
        assert float(w_mle[0, 2]) == 0.0
        m = _objective(family, 0.3, w=(1.0, 0.0, 0.0))
        _, g = m.value_and_grad(x, td, ed, log_logit_scale=torch.tensor(C.LOG_LOGIT_SCALE, device=DEV))
        assert g[0, 2].item() == 0.0
    if family == "hazard" and name == "survival-below-eps":
        m = _objective(family, 0.3, w=(1.0, 0.0, 0.0))
        _, g = m.value_and_grad(x, td, ed, log_logit_scale=torch.tensor(C.LOG_LOGIT_SCALE, device=DEV))
        assert not bool(g[1].any()) and not bool(g[0, :2].any()) and g[0, 2].item() != 0.0      # censored: nothing; event: only -log h_t
    if name == "t-outside-the-bins":        # clamped into [0, K - 1]: the same bits as the clamped labels
        v2, g2 = obj.value_and_grad(x, td.clamp(0, K - 1), ed, log_logit_scale=torch.tensor(C.LOG_LOGIT_SCALE, device=DEV))
        assert _same_bits(g2, grad)


# ---- 3. the modules: the per-sample entry on given hazards, SurvT2I alone
@pytest.mark.parametrize("K,B", C.ROW_SHAPES)
def test_per_sample_values_and_gradient_rows_on_given_hazards(K, B):
    from vlsa_amd import _native as nat
    from vlsa_amd import losses as L
    h, t, e = C.row_inputs(K, B)
    hd, td, ed = _dev(h, t, e)
    for which in ("mle", "emd"):
        values, rows = C.row_truth(K, B, which)
        w = (1.0, 0.0) if which == "mle" else (0.0, 1.0)
        o1, o2, g = L._launch_terms(hd, td, ed, nat.CONV_NONE, nat.SURV_MLE, C.ROW_LOGIT_SCALE, 0.0, C.EPS, 2, True, w[0], w[1], want_grad=True)
        got = o1 if which == "mle" else o2
        ev, eg = C.rel_value_rows(got.cpu(), values), S.rel_grad_rows(g.cpu(), rows)
        print(f"K={K} B={B} {which}: per-sample values {ev:.2e} (gate {C.ROW_VALUE_RTOL:g}); gradient rows, each rel to its own max: {eg:.2e} "
              f"(gate {C.ROW_GRAD_RTOL:g})")
        assert ev <= C.ROW_VALUE_RTOL and eg <= C.ROW_GRAD_RTOL
    # the module: the mean, differentiable w.r.t. the hazards, cur_alpha overriding alpha
    values, rows = C.row_truth(K, B, "mle")
    xd = hd.clone().requires_grad_(True)
    got = L.SurvMLE()(xd, td.view(-1, 1), ed.view(-1, 1))
    (2.0 * got).backward()
    assert got.shape == () and C.rel_value(got.item(), values.mean()) <= C.ROW_VALUE_RTOL
    assert S.rel_grad_rows(xd.grad.cpu(), 2.0 * rows / B) <= C.ROW_GRAD_RTOL
    a = L.SurvMLE(alpha=0.0)(hd, td, ed, cur_alpha=0.3)
    assert C.rel_value(a.item(), C.mle_rows(h.double(), 1 - h.double(), t, e, 0.3).mean()) <= C.ROW_VALUE_RTOL
    assert _same_bits(a, L.SurvMLE(alpha=0.3)(hd, td, ed))


@pytest.mark.parametrize("case", C.T2I_ALONE, ids=[f"k{c[0]}-b{c[1]}-{c[2]}-{c[3]}-ls{c[4]:g}" for c in C.T2I_ALONE])
def test_t2i_alone_against_float64(case):
    """vlsa_surv_t2i (a workgroup per bin, then a pass over the elements); KL also at a small logit scale, where the targets of the
    non-positives do not vanish"""
    from vlsa_amd.losses import SurvT2I
    K, B, loss, reduction, ls = case
    i, w64 = C.make_inputs("hazard", B, K, 8000 + 100 * K + B, 2.0), C.t2i_alone_truth(*case)
    x, t, e = _dev(i.logits, i.t, i.e)
    m = SurvT2I(loss=loss, reduction=reduction)
    xd = x.clone().requires_grad_(True)
    got = m(xd, t.view(-1, 1), e.view(-1, 1), torch.tensor(ls, device=DEV))
    got.backward()
    ev, eg = C.rel_value(got.detach().cpu(), w64.t2i), C.rel_grad(xd.grad.cpu(), w64.grad)
    print(f"T2I {loss}/{reduction} ls={ls:g} K={K} B={B}: value {ev:.2e} (gate {C.T2I_VALUE_RTOL:g}) gradient {eg:.2e} (gate {C.T2I_GRAD_RTOL:g})")
    assert got.shape == () and ev <= C.T2I_VALUE_RTOL and eg <= C.T2I_GRAD_RTOL
    x2 = x.clone().requires_grad_(True)                                                      # two runs: the same bits
    got2 = m(x2, t, e, ls)
    got2.backward()
    assert _same_bits(got2, got) and _same_bits(x2.grad, xd.grad)


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("K,B", [(12, 33), (17, 130), (16, C.ONE_BLOCK_MAX_B + 1)])
def test_two_runs_give_the_same_bits(family, K, B):
    i = C.make_inputs(family, B, K, 5000 + 100 * K + B, 2.0)
    x, t, e = _dev(i.logits, i.t, i.e)
    obj = _objective(family, 0.3, t2i_loss="KL")
    ls_log = torch.tensor(C.LOG_LOGIT_SCALE, device=DEV)
    v1, g1 = obj.value_and_grad(x, t, e, log_logit_scale=ls_log)
    v2, g2 = obj.value_and_grad(x.clone(), t, e, log_logit_scale=ls_log)
    assert _same_bits(v1, v2) and _same_bits(g1, g2)


# ---- 4. the default route is the launch it was
@pytest.mark.parametrize("K,B", [(12, 32), (17, 33)])
def test_default_objective_is_the_direct_call_of_vlsa_surv_objective(K, B):
    from vlsa_amd.losses import SurvObjective
    i = S.make_inputs(B, K, 5000 + 100 * K + B, 2.0)
    x, t, e = _dev(i.logits, i.t, i.e)
    ls_log = torch.tensor(C.LOG_LOGIT_SCALE, device=DEV)
    out = _direct_objective(x, t, e, ls_log, 0.0, 1e-7, 2, True, 1.0, 1.0)
    obj = SurvObjective()
    xd = x.clone().requires_grad_(True)
    got = obj(xd, t, e, log_logit_scale=ls_log)
    got.backward()
    assert torch.equal(got.detach(), out[0]) and torch.equal(xd.grad, out[1:].view(B, K))
    v, g = obj.value_and_grad(x, t, e, log_logit_scale=ls_log)
    assert torch.equal(v, out[0]) and torch.equal(g, out[1:].view(B, K))


@pytest.mark.parametrize("K", [12, 17])        # one per kernel; 33 samples: a full chunk plus one
def test_the_first_entry_points_forward_to_the_terms_launches(K):
    """vlsa_surv_loss and vlsa_surv_objective are forms of vlsa_surv_terms and vlsa_surv_objective_terms: the same bits"""
    from vlsa_amd import _native as nat
    B = 33
    i = S.make_inputs(B, K, 5000 + 100 * K + B, 2.0)
    x, t, e = _dev(i.logits, i.t, i.e)
    inc = torch.softmax(x, dim=-1)
    ls, ls_log = torch.tensor(C.LOGIT_SCALE, device=DEV), torch.tensor(C.LOG_LOGIT_SCALE, device=DEV)
    lib = nat.load()
    ptr = lambda v: ctypes.c_void_p(v.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    alpha, eps, p, raw, w1, w2 = 0.3, C.EPS, 2, 0, 0.7, 1.3

    def rows(call):
        o1, o2, g = torch.full((B,), float("nan"), device=DEV), torch.full((B,), float("nan"), device=DEV), torch.full((B, K), float("nan"), device=DEV)
        assert call(o1, o2, g) == 0
        assert bool(torch.isfinite(o1).all()) and bool(torch.isfinite(o2).all()) and bool(torch.isfinite(g).all())
        return o1, o2, g

    for pred, from_logits, conv in ((inc, 0, nat.CONV_NONE), (x, 1, nat.CONV_SOFTMAX)):
        old = rows(lambda o1, o2, g: lib.vlsa_surv_loss(ptr(pred), ptr(t), ptr(e), B, K, from_logits, ptr(ls), alpha, eps, p, raw, w1, w2, ptr(o1),
                                                        ptr(o2), ptr(g), stream))
        new = rows(lambda o1, o2, g: lib.vlsa_surv_terms(ptr(pred), ptr(t), ptr(e), B, K, conv, nat.SURV_IFMLE, ptr(ls), alpha, eps, p, raw, w1, w2,
                                                         ptr(o1), ptr(o2), ptr(g), stream))
        assert all(_same_bits(a, b) for a, b in zip(old, new)), from_logits
    for scale, is_log in ((ls, 0), (ls_log, 1)):
        old, new = (torch.full((1 + B * K,), float("nan"), device=DEV) for _ in range(2))
        assert lib.vlsa_surv_objective(ptr(x), ptr(t), ptr(e), B, K, 1, ptr(scale), is_log, alpha, eps, p, raw, w1, w2, ptr(old), ptr(old[1:]),
                                       stream) == 0
        assert lib.vlsa_surv_objective_terms(ptr(x), ptr(t), ptr(e), B, K, nat.CONV_SOFTMAX, nat.SURV_IFMLE, ptr(scale), is_log, alpha, eps, p, raw,
                                             w1, w2, 0.0, nat.T2I_CL, nat.T2I_MEAN, ptr(new), ptr(new[1:]), stream) == 0
        assert bool(torch.isfinite(old).all()) and _same_bits(old, new), is_log


# ---- 5. the entries refuse bad arguments before any launch (real buffers large enough for every variant, should one slip through)
def test_entries_refuse_bad_arguments():
    from vlsa_amd import _native as nat
    lib = nat.load()
    big = torch.zeros((nat.EVAL_MAX_M + 1) * (nat.MAX_K + 1), device=DEV)
    tt = torch.zeros(nat.EVAL_MAX_M + 1, dtype=torch.int64, device=DEV)
    ee = torch.zeros(nat.EVAL_MAX_M + 1, device=DEV)
    work = torch.zeros(5 * (nat.MAX_K + 1), dtype=torch.float64, device=DEV)
    out = torch.zeros_like(big)
    p, pt, pe, pw, po = (ctypes.c_void_p(v.data_ptr()) for v in (big, tt, ee, work, out))

    def call(fn, defaults, **k):
        assert set(k) <= {n for n, _ in defaults}
        return fn(*[k.get(n, d) for n, d in defaults])

    d_terms = (("x", p), ("t", pt), ("e", pe), ("B", 2), ("K", 4), ("conv", nat.CONV_SIGMOID), ("family", nat.SURV_MLE), ("ls", p), ("alpha", 0.0),
               ("eps", 1e-7), ("p", 2), ("raw", 1), ("w_main", 1.0), ("w_emd", 1.0), ("o1", None), ("o2", None), ("g", po), ("stream", None))
    terms = lambda **k: call(lib.vlsa_surv_terms, d_terms, **k)  # noqa: E731
    assert terms(x=None) == nat.EINVAL and terms(B=0) == nat.EINVAL and terms(K=0) == nat.EINVAL and terms(K=nat.MAX_K + 1) == nat.EINVAL
    assert terms(conv=3) == nat.EINVAL and terms(family=2) == nat.EINVAL and terms(ls=None) == nat.EINVAL
    assert terms(p=3) == nat.EUNSUPPORTED
    assert terms(conv=nat.CONV_SOFTMAX) == nat.EUNSUPPORTED and terms(family=nat.SURV_IFMLE) == nat.EUNSUPPORTED     # the handler's rule
    d_obj = (("x", p), ("t", pt), ("e", pe), ("B", 2), ("K", 4), ("conv", nat.CONV_SIGMOID), ("family", nat.SURV_MLE), ("ls", p), ("is_log", 0),
             ("alpha", 0.0), ("eps", 1e-7), ("p", 2), ("raw", 1), ("w_main", 1.0), ("w_emd", 1.0), ("w_t2i", 0.5), ("loss", nat.T2I_CL),
             ("red", nat.T2I_MEAN), ("out", po), ("g", po), ("stream", None))
    obj = lambda **k: call(lib.vlsa_surv_objective_terms, d_obj, **k)  # noqa: E731
    assert obj(out=None) == nat.EINVAL and obj(B=4097) == nat.EINVAL and obj(ls=None) == nat.EINVAL and obj(t=None) == nat.EINVAL
    assert obj(conv=nat.CONV_NONE) == nat.EINVAL                       # SurvT2I reads raw logits
    assert obj(loss=2) == nat.EUNSUPPORTED and obj(red=2) == nat.EUNSUPPORTED and obj(p=0) == nat.EUNSUPPORTED
    d_t2i = (("x", p), ("t", pt), ("e", pe), ("B", 2), ("K", 4), ("ls", p), ("is_log", 0), ("loss", nat.T2I_KL), ("red", nat.T2I_SUM), ("w", 1.0),
             ("work", pw), ("v", po), ("g", po), ("stream", None))
    t2i = lambda **k: call(lib.vlsa_surv_t2i, d_t2i, **k)  # noqa: E731
    assert t2i(work=None) == nat.EINVAL and t2i(v=None, g=None) == nat.EINVAL and t2i(ls=None) == nat.EINVAL and t2i(K=nat.MAX_K + 1) == nat.EINVAL
    assert t2i(B=nat.EVAL_MAX_M + 1) == nat.EUNSUPPORTED and t2i(loss=-1) == nat.EUNSUPPORTED and t2i(red=7) == nat.EUNSUPPORTED
    torch.cuda.synchronize()
    assert not bool(out.any())              # nothing was launched


# ---- 6. the evaluator
class _Loss:
    """stands in for a loss object of the reference: the attributes only"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.mark.parametrize("ours", [False, True], ids=["reference-shaped", "our-modules"])
@pytest.mark.parametrize("c", [c for c in C.FIXTURES if c.alpha == 0.3], ids=C.ids([c for c in C.FIXTURES if c.alpha == 0.3]))
def test_evaluator_against_the_references_dict(c, ours):
    from vlsa_amd import SurvEMD, SurvEvaluator, SurvIFMLE, SurvMLE, SurvT2I
    fx = C.load_fixture(c)
    raw, t, e = _dev(torch.from_numpy(fx["logits"]), torch.from_numpy(fx["t"]), torch.from_numpy(fx["e"]))
    hazard = c.family == "hazard"
    main_name = "SurvMLE" if hazard else "SurvIFMLE"
    if ours:
        losses = {main_name: SurvMLE(alpha=c.alpha, eps=C.EPS) if hazard else SurvIFMLE(alpha=c.alpha, eps=C.EPS),
                  "SurvEMD": SurvEMD(p=c.p, raw_distance=c.raw), "SurvT2I": SurvT2I(loss=c.t2i_loss, reduction=c.t2i_reduction)}
    else:
        losses = {main_name: _Loss(alpha=c.alpha, eps=C.EPS) if hazard else _Loss(alpha=c.alpha, eps=C.EPS, reduction="mean"),
                  "SurvEMD": _Loss(p=c.p, raw_distance=c.raw, reduction="mean"), "SurvT2I": _Loss(loss=c.t2i_loss, reduction=c.t2i_reduction)}
    keys = [str(k) for k in fx["eval_keys"]]
    metrics = [k for k in keys if not k.startswith("loss_Surv")]
    weight = {main_name: c.w_main, "SurvEMD": c.w_emd, "SurvT2I": c.w_t2i}
    data = {"y": torch.stack([t.float(), e], dim=1), "raw_y_hat": raw, "y_hat": torch.sigmoid(raw) if hazard else torch.softmax(raw, dim=-1), "uid": None}
    for ext in ([main_name, "SurvEMD", "SurvT2I"], ["SurvT2I"]):
        got = SurvEvaluator(c.family).compute(data, metrics, kws_ext_loss={n: losses[n] for n in ext}, loss_weight=weight,
                                              logit_scale=float(fx["logit_scale"]))
        assert list(got) == metrics + ["loss_" + n for n in ext]               # the reference's key order
        for k, v in got.items():
            assert isinstance(v, float)
            err = C.rel_value(v, fx["eval_" + k])
            print(f"{c.name} {'ours' if ours else 'stand-ins'} {k}: {v:.9g} reference {float(fx['eval_' + k]):.9g} rel {err:.2e}")
            assert err <= C.VALUE_RTOL[c.family], k
    # converted predictions alone (no raw logits) serve the per-sample terms too
    if hazard:
        del data["raw_y_hat"]
        got = SurvEvaluator("hazard").compute(data, ["loss"], kws_ext_loss={n: losses[n] for n in (main_name, "SurvEMD")}, loss_weight=weight,
                                              logit_scale=torch.tensor(float(fx["logit_scale"]), device=DEV))
        for k in ("loss_SurvMLE", "loss_SurvEMD"):
            assert C.rel_value(got[k], fx["eval_" + k]) <= C.ROW_VALUE_RTOL


# ---- 7. TrainStep under the hazard objective with SurvT2I: the tiny model and batches of tests/test_gpu_train_step_graph.py
K_TS, P_TS, TOWER, TSEED = 12, 12, "train", 9300


def _model():
    from vlsa_amd.prompt_adapter import PromptAdapter
    from vlsa_amd.prompt_encoder import CONCHPromptEncoder
    from vlsa_amd.prompt_learner import RankPromptLearner
    from vlsa_amd.vlsa import VLSA
    params = cases.make_params(P_TS, K_TS, 9201)
    c = TC.TOWERS[TOWER]
    enc = CONCHPromptEncoder(width=c["width"], heads=c["heads"], layers=c["layers"], vocab_size=c["vocab"], output_dim=c["out_dim"])
    enc.load_state_dict(TC.make_tower_weights(TOWER, TSEED))
    for p_ in enc.parameters():
        p_.requires_grad_(False)
    table, ctx_key, names = TC.synthetic_prompt_table(c["vocab"], TSEED)
    pl = RankPromptLearner(dict(max_num_tokens=127, embedding_dim=c["width"], embedding_dtype=torch.float32), TC.ReplayTokenizer(table),
                           enc.token_embedding, num_base_ranks=4, num_ranks=K_TS, num_tokens_per_rank=4, num_context_tokens=8,
                           init_context=ctx_key, init_rank_names=names)
    qnet = PromptAdapter(method="TaskRes", num_prompts=P_TS, pretrained_prompt_features=params["prompt"], res_ratio=0.5)
    cfg = dict(name="VLFAN", dim_in=512, use_feat_proj=False, num_query=P_TS, query="Text", query_pooling="mean", pred_head="default")
    net = VLSA.from_modules(cfg, prompt_learner=pl, prompt_encoder=enc, query_network=qnet, logit_scale_init=cases.LOGIT_SCALE).cuda().train()
    with torch.no_grad():
        qnet.residual_features.copy_(params["resid"])
        net.mil_encoder.visual_adapter.weight.copy_(params["W"])
        net.mil_encoder.visual_adapter.bias.copy_(params["b"])
    named = [net.mil_encoder.Q.residual_features, net.mil_encoder.visual_adapter.weight, net.mil_encoder.visual_adapter.bias,
             pl.context_embeds, pl.rank_embeds, net.logit_scale]
    return net, named


def _groups(ps):
    return [{"params": [p for p in ps if p.dim() < 2], "weight_decay": 0.0}, {"params": [p for p in ps if p.dim() >= 2], "weight_decay": 1e-5}]


def _batch():
    g = torch.Generator().manual_seed(77)
    bags = [cases.make_bag(int(torch.randint(200, 1500, (1,), generator=g)), 9600 + i, "clustered").to(torch.bfloat16).cuda() for i in range(8)]
    t = torch.randint(0, K_TS - 1, (8,), generator=g).cuda()
    e = (torch.rand(8, generator=g) < 0.5).float().cuda()
    return bags, t, e


def _run(graph, n_steps):
    from vlsa_amd.losses import SurvObjective
    from vlsa_amd.optim import FusedAdam
    from vlsa_amd.train_step import TrainStep
    net, named = _model()
    opt = FusedAdam(_groups(named), lr=1e-3)
    obj = SurvObjective(weight_ifmle=0, weight_mle=1, weight_emd=1, weight_t2i=0.5, converter="sigmoid")
    ts = TrainStep(net, obj, opt, graph=graph)
    bags, t, e = _batch()
    assert bool(e.any())                # SurvT2I counts a bin
    losses = []
    for i in range(n_steps):
        v0 = [p._version for p in named]
        losses.append(float(ts.step(bags, t, e)))
        assert all(p._version > v for p, v in zip(named, v0)), i
    return losses, [p.detach().clone() for p in named], ts


def test_train_step_replays_the_hazard_objective_with_t2i():
    le, pe, _ = _run(False, 12)
    lg, pg, ts = _run(True, 12)
    d = ts.describe()
    assert d["replays"] >= 9 and d["captures"] == 1 and d["why_eager"] is None, d
    assert le[0] != le[-1] and all(abs(v) < 1e4 for v in le)
    for a, b in zip(le, lg):
        assert abs(a - b) <= 2e-6 * max(1.0, abs(a)), (le, lg)
    for a, b in zip(pe, pg):
        assert (a - b).abs().max().item() <= 2e-6 * max(1.0, a.abs().max().item())
