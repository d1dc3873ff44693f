"""CPU side of the tests of the handler's other objectives (hazard family, SurvT2I): the float64 restatement of tests/objective_cases.py is
pinned to the reference's own float64 results (tests/golden/objective_*.npz), every case's inputs keep the conditions that make a float64
comparison meaningful, the gates the GPU tests apply are measured as 8 x the worst error of a plain fp32 evaluation of the same
formulas, and the Python layer constructs, refuses and binds what it should -- all without a GPU."""
import functools
import math
import os
import re
from ctypes import c_float, c_int, c_void_p

import pytest
import torch

import objective_cases as C
import surv_eval_helpers as H
import surv_loss_cases as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_constants_match_the_source():
    from vlsa_amd import _native as nat
    src = open(os.path.join(REPO, "vlsa_amd", "csrc", "surv_objectives.hip")).read()

    def const(name):
        return int(re.search(rf"\b{name} = (\d+)\b", src).group(1))

    assert C.MAX_K == nat.MAX_K and C.ROWS16_MAX_K < C.MAX_K and src.count("if (a.K <= 16)") == 1 and C.ROWS16_MAX_K == 16
    assert C.CHUNK == const("kTermThreads") == const("kTermWide") // 16 and "kTermWideSamples = kTermWide / 16" in src
    assert C.T2I_GROUPS_ROWS16 == const("kTermWide") // 16
    assert C.T2I_GROUPS_WIDE == const("kTermBlock") // const("kTermCols") and const("kTermCols") == nat.MAX_K
    assert C.T2I_GROUPS_ALONE == const("kT2iThreads")
    assert src.count("B > kOneBlockMaxB") == 2 and C.ONE_BLOCK_MAX_B == S.ONE_BLOCK_MAX_B == const("kOneBlockMaxB") == 4096
    from vlsa_amd import losses
    assert losses.ONE_LAUNCH_MAX_B == C.ONE_BLOCK_MAX_B
    assert nat.EVAL_MAX_M == 65536 and "B > VLSA_EVAL_MAX_M" in src


def test_case_tables_hold_what_the_kernels_branch_on():
    assert len({c.name for c in C.OBJECTIVE_CASES + C.FIXTURES}) == len(C.OBJECTIVE_CASES) + len(C.FIXTURES)
    for family in C.FAMILIES:
        grid = [c for c in C.GRID if c.family == family]
        assert {c.K for c in grid} == {1, 2, C.ROWS16_MAX_K - 1, C.ROWS16_MAX_K, C.ROWS16_MAX_K + 1, C.MAX_K - 1, C.MAX_K}
        want_b = {1, 130} | {g + d for g in (C.CHUNK, C.T2I_GROUPS_ROWS16, C.T2I_GROUPS_WIDE) for d in (-1, 0, 1)}
        assert {c.B for c in grid} == want_b and {c.t2i_loss for c in grid} == {"CL", "KL"}
        assert {(c.K, c.B) for c in C.BIG if c.family == family} == {(K, C.ONE_BLOCK_MAX_B + d) for K in (16, 17) for d in (-1, 0, 1)}
        assert {c.K for c in C.EXTREME if c.family == family} == {16, 17, 64} and all(c.scale == 12.0 and c.B == 130 for c in C.EXTREME)
        opts = [c for c in C.OPTIONS if c.family == family]
        assert {c.alpha for c in opts} == {0.0, 0.3} and {(c.p, c.raw) for c in opts} == {(2, True), (2, False), (1, True)}
        assert {c.t2i_reduction for c in opts} == {"mean", "sum"}
        for j in range(3):       # a zero for each term
            assert any((c.w_main, c.w_emd, c.w_t2i)[j] == 0 for c in opts)
        fx = [c for c in C.FIXTURES if c.family == family]
        assert {(c.B, c.K) for c in fx} == {(1, 4), (5, 12), (33, 16), (33, 17), (130, 64)}
        assert {(c.alpha, c.t2i_reduction) for c in fx} == {(a, r) for a in (0.0, 0.3) for r in ("mean", "sum")}
    assert all(c.all_events == (c.p == 2 and not c.raw) for c in C.OBJECTIVE_CASES)
    assert C.fixture_files() == sorted({C.fixture_file(c) for c in C.FIXTURES}) and len(C.fixture_files()) == 10
    assert all(os.path.getsize(os.path.join(H.GOLDEN, f)) < 512 * 1024 for f in C.fixture_files())


# ---- the restatement against the reference's own float64 results
def _close(got, want, rtol=1e-10):
    return abs(float(got) - float(want)) <= rtol * abs(float(want))


@pytest.mark.parametrize("c", C.FIXTURES, ids=C.ids(C.FIXTURES))
def test_restatement_has_the_references_float64_results(c):
    fx, i = C.load_fixture(c), C.case_inputs(c)
    assert torch.equal(torch.from_numpy(fx["logits"]), i.logits) and fx["logits"].dtype.name == "float32"
    assert torch.equal(torch.from_numpy(fx["t"]), i.t) and torch.equal(torch.from_numpy(fx["e"]), i.e)
    assert str(fx["family"]) == c.family and str(fx["t2i_loss"]) == c.t2i_loss and str(fx["t2i_reduction"]) == c.t2i_reduction
    assert (float(fx["alpha"]), int(fx["p"]), bool(fx["raw_distance"])) == (c.alpha, c.p, c.raw)
    assert (float(fx["w_main"]), float(fx["w_emd"]), float(fx["w_t2i"])) == (c.w_main, c.w_emd, c.w_t2i)
    ls = float(fx["logit_scale"])
    r = C.truth(i.logits, i.t, i.e, ls, c.family, c.alpha, float(fx["eps"]), c.p, c.raw, c.w_main, c.w_emd, c.w_t2i, c.t2i_loss, c.t2i_reduction)
    assert r.slots == int(fx["t2i_slots"])
    assert _close(r.main.mean(), fx["ref64_main"]) and _close(r.emd.mean(), fx["ref64_emd"]) and _close(r.objective, fx["ref64_total"])
    assert _close(r.t2i, fx["ref64_t2i"]) if r.slots else (float(r.t2i) == 0.0 == float(fx["ref64_t2i"]))
    want = torch.from_numpy(fx["ref64_grad"])
    assert r.grad.dtype == torch.float64 and float((r.grad - want).abs().max()) <= 1e-10 * float(want.abs().max())
    # the evaluator's dict: the metrics in the order asked, then loss_<name> in the order of the handler's loss dict
    main_name = "SurvMLE" if c.family == "hazard" else "SurvIFMLE"
    ext = [main_name, "SurvEMD"] + (["SurvT2I"] if r.slots else [])
    metrics = ["c_index", "loss", "loss_mle", "loss_mle_org"] if bool(i.e.any()) and c.B >= 2 else ["loss", "loss_mle", "loss_mle_org"]
    assert [str(k) for k in fx["eval_keys"]] == metrics + ["loss_" + n for n in ext]
    ev = H.evaluate(i.logits, i.t, i.e, c.family)
    for m in metrics:
        assert _close(ev[m], fx["eval_" + m]), m
    assert _close(c.w_main * r.main.mean(), fx["eval_loss_" + main_name]) and _close(c.w_emd * r.emd.mean(), fx["eval_loss_SurvEMD"])
    if r.slots:
        assert _close(c.w_t2i * r.t2i, fx["eval_loss_SurvT2I"])


def test_t2i_restatement_handles_what_the_reference_loops_over():
    x, t, e = C.EDGES["bin-without-a-positive"](5)
    part, pos = C.t2i_bins(t, e, 5)
    assert part[:, 0].tolist() == [True, True, True, True] and not bool(pos[:, 0].any())            # participants, no positive
    assert part[1].tolist() == [True, True, False, False, False] and not bool(pos[1].any())         # censored, t = 2: bins 0 and 1
    assert C.t2i_value(x.double(), t, e, 2.0, "CL")[1] == 2                                          # bins 1 and 3
    v, slots = C.t2i_value(x[:1].double(), torch.tensor([1]), torch.tensor([1.0]), 2.0, "CL")          # one event: log-softmax of one entry
    assert slots == 1 and float(v) == 0.0
    v, slots = C.t2i_value(x.double(), t, torch.zeros(4), 2.0, "KL")
    assert slots == 0 and float(v) == 0.0 and v.dtype == torch.float64


# ---- inputs
@pytest.mark.parametrize("c", C.OBJECTIVE_CASES + C.FIXTURES, ids=C.ids(C.OBJECTIVE_CASES + C.FIXTURES))
def test_inputs_keep_their_rule_and_cap(c):
    i = C.case_inputs(c)
    assert i.logits.shape == (c.B, c.K) and i.logits.dtype == torch.float32 and i.t.dtype == torch.int64 and i.e.dtype == torch.float32
    assert int(i.t.min()) >= 0 and int(i.t.max()) < c.K
    assert i.changed <= C.MAX_ALTERED * c.B or c.K < 15, i.changed       # (the cap of surv_loss_cases.py: from 15 bins on)
    cen = i.e == 0
    if c.family == "hazard":
        assert not bool(C.in_band(i.logits, i.t, i.e).any())             # the rule held
        assert i.changed <= C.MAX_ALTERED * c.B
        y = torch.sigmoid(i.logits.double())
    else:
        y = torch.softmax(i.logits.double(), dim=-1)
        if c.K >= 2:
            tail = 1.0 - torch.cumsum(y, dim=-1).gather(1, i.t.view(-1, 1)).view(-1)
            assert bool((tail[cen] >= S.MIN_TAIL).all())
        a = y.gather(1, i.t.view(-1, 1)).view(-1)[~cen]
        assert not bool(((a >= 0.5e-7) & (a <= 2e-7)).any())
    if c.p == 1:        # |d| has a kink at 0: no cdf difference of an event below the last bin within fp32 rounding of it
        k = torch.arange(c.K).view(1, c.K)
        target = ((k == i.t.view(-1, 1)).long() + (k > i.t.view(-1, 1)).long() * (1 - i.e.view(-1, 1).long())).double()
        pred = torch.where(cen.view(-1, 1), (1 - target) * y + target * C.LOGIT_SCALE, y)
        d = torch.cumsum(torch.softmax(pred, dim=-1), dim=-1) - torch.cumsum(torch.softmax((2 * target - 1) * C.LOGIT_SCALE, dim=-1), dim=-1)
        assert float(d[~cen][:, :c.K - 1].abs().min()) >= 1e-6
    # SurvT2I: at least one counted bin, except where the draw holds no event
    slots = C.case_truth(c).slots
    if c in C.GRID and (c.K, c.B) in C.GRID_WITHOUT_COUNTED_BIN:
        assert slots == 0 and not bool(i.e.any())
    else:
        assert slots >= 1


@pytest.mark.parametrize("family", C.FAMILIES)
def test_edge_inputs_are_the_edges_they_are_named_for(family):
    for K in C.EDGE_BINS:
        for name in C.EDGE_NAMES[family]:
            x, t, e = C.EDGES[name](K)
            slots = C.edge_truth(name, K, family, "CL").slots
            assert (slots == 0) == (name in C.NO_COUNTED_BIN), name
            tc = t.clamp(0, K - 1)
            if family == "hazard":
                assert not bool(C.in_band(x, t, e).any())
            else:
                tail = 1.0 - torch.cumsum(torch.softmax(x.double(), dim=-1), dim=-1).gather(1, tc.view(-1, 1)).view(-1)
                assert bool((tail[e == 0] >= S.MIN_TAIL).all()), name
        q = C.clamped_quantities(*C.EDGES["h-below-eps"](K))
        assert float(q[0, 0]) < C.EPS / 10 and float(q[0, 1]) > 10 * C.EPS                  # h_t clamped, S_padded[t] not
        q = C.clamped_quantities(*C.EDGES["survival-below-eps"](K))
        assert float(q[0, 1]) < C.EPS / 10 and float(q[0, 0]) > 10 * C.EPS and float(q[1, 0]) < C.EPS / 10
        g = C.edge_truth("h-below-eps", K, "hazard", "CL").grad
        assert bool(torch.isfinite(g).all())
        t = C.EDGES["t-outside-the-bins"](K)[1]
        assert int(t.min()) < 0 and int(t.max()) > K - 1
        g = C.edge_truth("censored-at-t0", K, family, "CL")
        assert g.slots >= 1


# ---- the gates
@functools.lru_cache(maxsize=None)
def _objective_errors(c):
    want, got = C.case_truth(c), C.case_truth(c, torch.float32)
    return C.rel_value(got.objective, want.objective), C.rel_grad(got.grad, want.grad)


@functools.lru_cache(maxsize=None)
def _edge_errors(name, K, family, loss):
    want, got = C.edge_truth(name, K, family, loss), C.edge_truth(name, K, family, loss, torch.float32)
    return C.rel_value(got.objective, want.objective), C.rel_grad(got.grad, want.grad)


@functools.lru_cache(maxsize=None)
def _row_errors(K, B, which):
    (v64, g64), (v32, g32) = C.row_truth(K, B, which), C.row_truth(K, B, which, torch.float32)
    return C.rel_value_rows(v32, v64), S.rel_grad_rows(g32, g64)


_EDGE_CASES = [(n, K, f, loss) for f in C.FAMILIES for n in C.EDGE_NAMES[f] for K in C.EDGE_BINS for loss in ("CL", "KL")]


@pytest.mark.parametrize("c", C.OBJECTIVE_CASES + C.FIXTURES, ids=C.ids(C.OBJECTIVE_CASES + C.FIXTURES))
def test_fp32_restatement_of_the_objective_stays_within_an_eighth_of_the_gates(c):
    """(the scale-12 table included: written with sigmoid(-x), a plain fp32 evaluation meets the same gates there)"""
    ev, eg = _objective_errors(c)
    print(f"{c.name}: fp32 restatement value {ev:.2e} (gate {C.VALUE_RTOL[c.family]:g}) gradient {eg:.2e} (gate {C.GRAD_RTOL[c.family]:g})")
    assert ev <= C.VALUE_RTOL[c.family] / 8 and eg <= C.GRAD_RTOL[c.family] / 8


@pytest.mark.parametrize("name,K,family,loss", _EDGE_CASES)
def test_fp32_restatement_of_the_edges_stays_within_an_eighth_of_the_gates(name, K, family, loss):
    ev, eg = _edge_errors(name, K, family, loss)
    assert ev <= C.VALUE_RTOL[family] / 8 and eg <= C.GRAD_RTOL[family] / 8


@pytest.mark.parametrize("which", ["mle", "emd"])
@pytest.mark.parametrize("K,B", C.ROW_SHAPES)
def test_fp32_restatement_of_the_per_sample_route_stays_within_an_eighth_of_the_gates(K, B, which):
    ev, eg = _row_errors(K, B, which)
    assert ev <= C.ROW_VALUE_RTOL / 8 and eg <= C.ROW_GRAD_RTOL / 8


@functools.lru_cache(maxsize=None)
def _t2i_alone_errors(case):
    want, got = C.t2i_alone_truth(*case), C.t2i_alone_truth(*case, dtype=torch.float32)
    assert want.slots >= 1
    return C.rel_value(got.t2i, want.t2i), C.rel_grad(got.grad, want.grad)


@pytest.mark.parametrize("case", C.T2I_ALONE, ids=[f"k{c[0]}-b{c[1]}-{c[2]}-{c[3]}-ls{c[4]:g}" for c in C.T2I_ALONE])
def test_fp32_restatement_of_t2i_alone_stays_within_an_eighth_of_the_gates(case):
    ev, eg = _t2i_alone_errors(case)
    assert ev <= C.T2I_VALUE_RTOL / 8 and eg <= C.T2I_GRAD_RTOL / 8


def test_subtracting_the_sigmoid_from_one_misses_the_gate_at_scale_12():
    """why the kernels form 1 - h as sigmoid(-x): the same fp32 evaluation with 1 - sigmoid(x) misses the gate itself"""
    worst = 0.0
    for c in C.EXTREME:
        if c.family == "hazard" and c.t2i_loss == "CL":
            i = C.case_inputs(c)
            h = torch.sigmoid(i.logits)
            worst = max(worst, C.rel_value(C.mle_rows(h, 1 - h, i.t, i.e).mean(), C.case_truth(c).main.mean()))
    assert worst > C.VALUE_RTOL["hazard"], worst


def _round_up_one_digit(v):
    m = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / m - 1e-9) * m


def test_gates_are_eight_times_the_fp32_restatement():
    """the gates of objective_cases.py are 8 x the worst figure over every case of a family (tables, fixtures, edges), rounded up to one
    significant digit -- no tighter (a correct fp32 kernel reaches them) and no looser"""
    worst = {}

    def note(kind, err, where):
        if err > worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (err, where)

    for c in C.OBJECTIVE_CASES + C.FIXTURES:
        ev, eg = _objective_errors(c)
        note(("value", c.family), ev, c.name)
        note(("gradient", c.family), eg, c.name)
    for (n, K, f, loss) in _EDGE_CASES:
        ev, eg = _edge_errors(n, K, f, loss)
        note(("value", f), ev, f"{n} K={K} {loss}")
        note(("gradient", f), eg, f"{n} K={K} {loss}")
    for K, B in C.ROW_SHAPES:
        for w in ("mle", "emd"):
            ev, eg = _row_errors(K, B, w)
            note("row values", ev, f"{w} K={K} B={B}")
            note("row gradients", eg, f"{w} K={K} B={B}")
    for case in C.T2I_ALONE:
        ev, eg = _t2i_alone_errors(case)
        note("t2i alone values", ev, str(case))
        note("t2i alone gradients", eg, str(case))
    for kind, (err, where) in worst.items():
        print(f"worst fp32 restatement error, {kind}: {err:.3e} at {where} -> gate {_round_up_one_digit(8 * err):g}")
    for f in C.FAMILIES:
        assert math.isclose(C.VALUE_RTOL[f], _round_up_one_digit(8 * worst[("value", f)][0]), rel_tol=1e-9)
        assert math.isclose(C.GRAD_RTOL[f], _round_up_one_digit(8 * worst[("gradient", f)][0]), rel_tol=1e-9)
    assert math.isclose(C.ROW_VALUE_RTOL, _round_up_one_digit(8 * worst["row values"][0]), rel_tol=1e-9)
    assert math.isclose(C.ROW_GRAD_RTOL, _round_up_one_digit(8 * worst["row gradients"][0]), rel_tol=1e-9)
    assert math.isclose(C.T2I_VALUE_RTOL, _round_up_one_digit(8 * worst["t2i alone values"][0]), rel_tol=1e-9)
    assert math.isclose(C.T2I_GRAD_RTOL, _round_up_one_digit(8 * worst["t2i alone gradients"][0]), rel_tol=1e-9)


# ---- the Python layer, without a GPU
class _Loss:
    """stands in for a loss object of either code base: the attributes only"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_objective_construction_and_refusals():
    from vlsa_amd import SurvObjective, _native as nat
    o = SurvObjective()
    assert (o.converter, o.w_mle, o.w_t2i, o.t2i_loss, o.t2i_reduction) == ("softmax", 0.0, 0.0, "CL", "mean")
    assert o._spec() == (nat.CONV_SOFTMAX, nat.SURV_IFMLE, 0.0, 1e-7, 2, True, 1.0, 1.0, 0.0, "CL", "mean")
    # the positional arguments are the old ones
    assert SurvObjective(0.5, 2.0, 0.3, 1e-6, 1, False)._spec() == (nat.CONV_SOFTMAX, nat.SURV_IFMLE, 0.3, 1e-6, 1, False, 0.5, 2.0, 0.0, "CL", "mean")
    with pytest.raises(TypeError):
        SurvObjective(1.0, 1.0, 0.0, 1e-7, 2, True, "sigmoid")                      # the new ones are keyword-only
    with pytest.raises(ValueError, match="softmax"):
        SurvObjective(converter="sigmoid")                                          # weight_ifmle defaults to 1
    with pytest.raises(ValueError, match="sigmoid"):
        SurvObjective(weight_mle=1.0)
    with pytest.raises(ValueError):
        SurvObjective(converter="none")
    with pytest.raises(NotImplementedError):
        SurvObjective(weight_t2i=1.0, t2i_loss="MSE")
    with pytest.raises(NotImplementedError):
        SurvObjective(p=3)
    o = SurvObjective(weight_ifmle=0, weight_mle=1, weight_emd=1, weight_t2i=0.5, converter="sigmoid")
    assert o._spec() == (nat.CONV_SIGMOID, nat.SURV_MLE, 0.0, 1e-7, 2, True, 1, 1, 0.5, "CL", "mean")
    o = SurvObjective(weight_t2i=0.25, t2i_loss="KL", t2i_reduction="sum")
    assert o._spec()[:2] == (nat.CONV_SOFTMAX, nat.SURV_IFMLE) and o._spec()[-3:] == (0.25, "KL", "sum")


def test_from_handler_reads_either_code_bases_objects():
    from vlsa_amd import SurvEMD, SurvMLE, SurvObjective, SurvT2I, _native as nat
    standins = {"SurvMLE": _Loss(alpha=0.3, eps=1e-6), "SurvEMD": _Loss(p=1, raw_distance=True, reduction="mean"),
                "SurvT2I": _Loss(loss="KL", reduction="sum")}
    ours = {"SurvMLE": SurvMLE(alpha=0.3, eps=1e-6), "SurvEMD": SurvEMD(p=1), "SurvT2I": SurvT2I(loss="KL", reduction="sum")}
    weight = {"SurvMLE": 1.0, "SurvEMD": 0.7, "SurvT2I": 0.2}
    for loss in (standins, ours):
        o = SurvObjective.from_handler(loss, weight, "sigmoid")
        assert o._spec() == (nat.CONV_SIGMOID, nat.SURV_MLE, 0.3, 1e-6, 1, True, 1.0, 0.7, 0.2, "KL", "sum")
    o = SurvObjective.from_handler({"SurvIFMLE": _Loss(alpha=0.0, eps=1e-7, reduction="mean"), "SurvEMD": _Loss(p=2, raw_distance=False, reduction="mean")},
                                   {"SurvIFMLE": 1.0, "SurvEMD": 1.0}, "softmax")
    assert o._spec() == (nat.CONV_SOFTMAX, nat.SURV_IFMLE, 0.0, 1e-7, 2, False, 1.0, 1.0, 0.0, "CL", "mean")
    with pytest.raises(ValueError):         # the handler's rule
        SurvObjective.from_handler({"SurvMLE": _Loss(alpha=0.0, eps=1e-7)}, {"SurvMLE": 1.0}, "softmax")
    for bad in ({"QueryDiv": _Loss()}, {"SurvEMD": _Loss(p=3, raw_distance=True, reduction="mean")},
                {"SurvEMD": _Loss(p=2, raw_distance=True, reduction="sum")}, {"SurvIFMLE": _Loss(alpha=0.0, eps=1e-7, reduction="none")},
                {"SurvT2I": _Loss(loss="MSE", reduction="mean")}):
        with pytest.raises(NotImplementedError):
            SurvObjective.from_handler(bad, {n: 1.0 for n in bad}, "softmax")


def test_modules_keep_the_references_signatures():
    from vlsa_amd import SurvMLE, SurvT2I
    m = SurvMLE(alpha=0.2, eps=1e-6, reduction="ignored")
    assert (m.alpha, m.eps) == (0.2, 1e-6) and (SurvMLE().alpha, SurvMLE().eps) == (0.0, 1e-7)
    t = SurvT2I()
    assert (t.loss, t.reduction) == ("CL", "mean") and SurvT2I("KL", "sum", extra=1).loss == "KL"
    with pytest.raises(NotImplementedError, match="CL or KL"):
        SurvT2I(loss="MSE")
    assert "zero" in SurvT2I.__doc__ and "0.0" in SurvT2I.__doc__                 # the one stated difference from the reference


def test_cpu_tensors_are_refused():
    from vlsa_amd import SurvEvaluator, SurvMLE, SurvObjective, SurvT2I, VlsaNativeError
    x, t, e = torch.zeros(2, 4), torch.tensor([0, 1]), torch.tensor([1.0, 0.0])
    with pytest.raises(VlsaNativeError):
        SurvMLE()(torch.sigmoid(x), t, e)
    with pytest.raises(VlsaNativeError):
        SurvT2I()(x, t, e)
    o = SurvObjective(weight_ifmle=0, weight_mle=1, weight_t2i=0.5, converter="sigmoid")
    with pytest.raises(VlsaNativeError):
        o(x, t, e, cur_logit_scale=torch.tensor(10.0))
    with pytest.raises(VlsaNativeError):
        o.value_and_grad(x, t, e, log_logit_scale=torch.tensor(2.0))
    data = {"y": torch.stack([t.float(), e], dim=1), "raw_y_hat": x, "uid": None}
    with pytest.raises(VlsaNativeError):
        SurvEvaluator("hazard").compute(data, ["loss"], kws_ext_loss={"SurvMLE": _Loss(alpha=0.0, eps=1e-7)})


def test_evaluator_refuses_what_the_launches_do_not_cover():
    from vlsa_amd import SurvEvaluator
    data = {"y": torch.tensor([[0.0, 1.0], [1.0, 0.0]]), "raw_y_hat": torch.zeros(2, 2)}
    for ptype, losses in [("hazard", {"SurvEMD": _Loss(p=3, raw_distance=True, reduction="mean")}),
                          ("hazard", {"SurvEMD": _Loss(p=2, raw_distance=True, reduction="sum")}),
                          ("hazard", {"SurvIFMLE": _Loss(alpha=0.0, eps=1e-7, reduction="mean")}),
                          ("incidence", {"SurvT2I": _Loss(loss="MSE", reduction="mean")})]:
        with pytest.raises(NotImplementedError):       # (raised before a tensor is looked at)
            SurvEvaluator(ptype).compute(data, ["loss"], kws_ext_loss=losses)


# ---- the binding: typed by hand from the declarations of include/vlsa_hip.h (never pasted from the reader's output)
V, I, F = c_void_p, c_int, c_float
SPOT_SIGNATURES = {
    "vlsa_surv_terms": (I, [V, V, V, I, I, I, I, V, F, F, I, I, F, F, V, V, V, V]),
    "vlsa_surv_objective_terms": (I, [V, V, V, I, I, I, I, V, I, F, F, I, I, F, F, F, I, I, V, V, V]),
    "vlsa_surv_t2i": (I, [V, V, V, I, I, V, I, I, I, F, V, V, V, V]),
}


@pytest.mark.parametrize("name", sorted(SPOT_SIGNATURES))
def test_derived_signature_equals_the_hand_typed_one(name):
    from vlsa_amd import _native as nat
    assert nat._SIGNATURES[name] == SPOT_SIGNATURES[name]
    assert nat.ABI_VERSION == 1
    assert (nat.CONV_NONE, nat.CONV_SOFTMAX, nat.CONV_SIGMOID, nat.SURV_IFMLE, nat.SURV_MLE) == (0, 1, 2, 0, 1)
    assert (nat.T2I_CL, nat.T2I_KL, nat.T2I_SUM, nat.T2I_MEAN, nat.T2I_WORK_PER_BIN) == (0, 1, 0, 1, 5)
