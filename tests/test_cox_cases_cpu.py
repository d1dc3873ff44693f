"""CPU side of the tests of the continuous survival heads' objective (SurvPLE, rank_loss, recon_loss, MSE_loss): the float64
restatement of tests/cox_cases.py is pinned to the reference's own float64 results (tests/golden/cox_objective_*.npz), the identity the
kernel is built on holds, every case's inputs keep the input rule, the gates the GPU tests apply are measured as 8 x the worst error of
a plain fp32 evaluation of the same formulas, and the Python layer constructs, refuses and binds what it should -- all without a GPU."""
import functools
import math
import os
import re
from ctypes import c_double, c_int, c_void_p

import pytest
import torch

import cox_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_constants_match_the_source():
    from vlsa_amd import _native as nat
    src = open(os.path.join(REPO, "vlsa_amd", "csrc", "surv_pairs.hip")).read()

    def const(name):
        return int(re.search(rf"\b{name} = (\d+)\b", src).group(1))

    assert C.THREADS == const("kPairObjThreads") and C.OWNED == const("kPairObjOwned") and C.MAX_B == const("kPairObjMaxB") == nat.PAIR_MAX_B
    assert C.OWNED * C.THREADS == C.MAX_B and "B > kPairObjMaxB" in src
    assert C.WAVE == 64 and "(B + 63) / 64 * 64" in src
    assert const("kPairObjLdsPerSample") * C.MAX_B <= 160 * 1024           # the batch fits the LDS of a gfx950 CU
    assert "10.f" in src and C.CAP == 10.0
    assert "atomic" not in src.lower().replace("no atomics", "")


def test_case_tables_hold_what_the_launch_branches_on():
    names = [c.name for c in _ALL]
    assert {c.B for c in C.SPLIT_ROUTE} == {C.MAX_B + 1} and {c.times for c in C.SPLIT_ROUTE} == set(C.TIMES)
    assert len(set(names)) == len(names)
    want_b = {1, 2, 3, 130} | {g + d for g in (C.WAVE, C.THREADS) for d in (-1, 0, 1)} | {C.MAX_B - 1, C.MAX_B}
    assert want_b <= {c.B for c in C.GRID} and C.REFUSED_B == C.MAX_B + 1
    for B in {c.B for c in C.GRID}:
        assert {c.times for c in C.GRID if c.B == B} == set(C.TIMES)
    assert all((c.rank_norm == "l1") == (c.B <= C.L1_MAX_B) for c in C.GRID)
    # l1 where a thread owns several samples, and on the split route: recon_loss beside rank l2, rank_loss on stepped predictions
    for cases, sizes in ((C.L1_LARGE, {C.THREADS + 1, C.MAX_B}), (C.SPLIT_ROUTE, {C.MAX_B + 1})):
        assert {c.B for c in cases if c.recon_norm == "l1" and c.rank_norm == "l2" and c.w_recon != 0} == sizes
        assert {c.B for c in cases if c.rank_norm == "l1" and c.w_rank != 0 and c.pred_kind == "steps"} == sizes
    assert all(C.case_inputs(c).changed == 0 and c.w_recon == 0 for c in _ALL if c.pred_kind == "steps")
    assert {(c.times, c.censor) for c in C.CENSORED} == {(t, s) for t in C.TIMES for s in C.CENSOR[1:]}
    for j in range(4):                  # each term alone, in both norms
        alone = [c for c in C.OPTIONS if [w != 0 for w in (c.w_ple, c.w_rank, c.w_recon, c.w_mse)] == [k == j for k in range(4)]]
        assert {c.rank_norm for c in alone} == {"l1", "l2"}
    assert {c.mse_censored for c in C.OPTIONS} == {False, True} and {c.recon_alpha for c in C.OPTIONS} == {0.0, 0.3}
    assert {(c.B, c.times, c.rank_norm) for c in C.FIXTURES} == {(B, t, n) for B in (1, 5, 33, 130) for t in C.TIMES for n in ("l1", "l2")}
    assert C.fixture_files() == sorted({C.fixture_file(c) for c in C.FIXTURES}) and len(C.fixture_files()) == 8
    assert all(os.path.getsize(os.path.join(C.GOLDEN, f)) < 64 * 1024 for f in C.fixture_files())


# ---- the inputs
_ALL = C.CASES + C.SPLIT_ROUTE + C.FIXTURES


@pytest.mark.parametrize("c", _ALL, ids=C.ids(_ALL))
def test_inputs_keep_the_input_rule(c):
    i = C.case_inputs(c)
    assert i.pred.dtype == i.t.dtype == i.e.dtype == torch.float32 and i.pred.shape == i.t.shape == i.e.shape == (c.B,)
    assert not bool(C.in_band(i.pred, i.t, i.e, c).any())
    assert i.changed <= C.MAX_ALTERED * c.B, (i.changed, c.B)           # a condition on the seed, not a tolerance
    assert set(i.e.tolist()) <= {0.0, 1.0}
    ties = len(torch.unique(i.t)) < c.B
    assert ties == (c.times == "ties" and c.B > 3) or c.B <= 12
    if c.B >= 4:
        assert i.pred[0].item() == C.CAP and i.pred[1].item() > C.CAP
    if c.B >= 130:
        assert int((i.pred > C.CAP).sum()) >= 2
        if c.censor == "mixed":
            assert 0.25 <= 1.0 - float(i.e.mean()) <= 0.55             # about 40 % censored
    want = C.case_truth(c)
    if c.censor == "all-censored":
        assert not bool(i.e.any()) and want.pairs == 0 and float(want.ple) == 0.0
    if c.censor == "all-event":
        assert bool(i.e.all())
    if c.censor == "no-pair":
        assert bool(i.e.any()) and want.pairs == 0 and float(want.rank) == 0.0      # events, all at the largest time


def test_exact_kinks_sit_on_their_kinks():
    p, t, e = (x.double() for x in C.EDGES["pred-equals-t"])
    assert e[0] == 1 and p[0] - t[0] == 0
    p, t, e = (x.double() for x in C.EDGES["gamma-minus-d-is-zero"])
    assert e[0] == 0 and C.EDGE_CASE.recon_gamma - (p[0] - t[0]) == 0
    p, t, e = (x.double() for x in C.EDGES["rank-pair-on-the-kink"])
    assert e[0] == 1 and t[0] < t[1] and C.EDGE_CASE.rank_gamma + p[0] - p[1] == 0
    # torch's derivative there is 0: moving the sample off the kink by one part in a thousand changes the gradient by a whole unit
    g0 = C.edge_truth("pred-equals-t").grad
    moved = C.truth(C.EDGES["pred-equals-t"][0] + torch.tensor([1e-3, 0.0, 0.0]), *C.EDGES["pred-equals-t"][1:], C.EDGE_CASE).grad
    assert abs(float(moved[0] - g0[0])) > 0.1
    assert not bool(C.edge_truth("all-above-the-cap")._replace().grad.isnan().any())


# ---- the restatement against the reference's own float64 results
@pytest.mark.parametrize("c", C.FIXTURES, ids=C.ids(C.FIXTURES))
def test_restatement_reproduces_the_references_float64_results(c):
    fx = C.load_fixture(c)
    i = C.case_inputs(c)
    assert torch.equal(torch.from_numpy(fx["pred"]), i.pred) and torch.equal(torch.from_numpy(fx["t"]), i.t)
    assert torch.equal(torch.from_numpy(fx["e"]), i.e) and str(fx["norm"]) == c.rank_norm
    assert fx["weights"].tolist() == [c.w_ple, c.w_rank, c.w_recon, c.w_mse]
    assert (float(fx["rank_gamma"]), float(fx["recon_alpha"]), float(fx["recon_gamma"]), bool(fx["mse_censored"])) == \
        (c.rank_gamma, c.recon_alpha, c.recon_gamma, c.mse_censored)
    want = C.case_truth(c, fp32_weights=True)                           # the reference's fp32 pair weights: its numbers to 1e-12
    exact = C.case_truth(c)                                             # the truth the kernel is held to: the exact mean
    assert abs(float(exact.rank) - float(want.rank)) <= 6e-8 * abs(float(want.rank))
    assert want.pairs == int(fx["rank_pairs"])                          # counts exact
    for field, key in (("ple", "ref64_ple"), ("rank", "ref64_rank"), ("recon", "ref64_recon"), ("mse", "ref64_mse"), ("objective", "ref64_total")):
        got, ref = float(getattr(want, field)), float(fx[key])
        assert abs(got - ref) <= 1e-12 * max(1.0, abs(ref)), (field, got, ref)
    ref = torch.from_numpy(fx["ref64_grad"])
    assert float((want.grad - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1.0 / c.B)


# ---- the identity the kernel, its gradient and Breslow's baseline share
def _identity(pred, t, e):
    """(SurvPLE, d SurvPLE / d pred) by the two passes of csrc/surv_pairs.hip, in float64, with the shift by the largest theta"""
    pred, t, e = pred.double(), t.double(), e.double()
    B = pred.numel()
    theta = torch.minimum(pred, torch.tensor(C.CAP, dtype=torch.float64))
    mx = theta.max()
    ex = torch.exp(theta - mx)
    D = torch.stack([ex[t >= t[i]].sum() for i in range(B)])
    inv = torch.where(e != 0, e / D, torch.zeros_like(D))
    H = torch.stack([inv[t <= t[k]].sum() for k in range(B)])
    value = 0.0 - (e * (theta - mx - torch.log(D))).sum() / B
    grad = -(e - ex * H) / B * (pred <= C.CAP)
    return value, grad


@pytest.mark.parametrize("c", [c for c in C.CASES + C.FIXTURES if c.B <= 130 and c.w_ple != 0], ids=lambda c: c.name)
def test_the_two_pass_identity_is_survple_and_its_gradient(c):
    i = C.case_inputs(c)
    value, grad = _identity(i.pred, i.t, i.e)
    want = C.truth(i.pred, i.t, i.e, c._replace(w_ple=1.0, w_rank=0.0, w_recon=0.0, w_mse=0.0))
    assert abs(float(value - want.ple)) <= 1e-12 * max(1.0, abs(float(want.ple)))
    assert float((grad - want.grad).abs().max()) <= 1e-12 * max(float(want.grad.abs().max()), 1.0 / c.B)


def test_the_shifted_identity_survives_where_the_plain_fp32_sum_does_not():
    """wide-spread: exp(-90) next to exp(9) -- in fp32 the small terms vanish from an unshifted risk-set sum only when they share it with
    the large one; the identity keeps each D_i to full precision and matches the float64 truth"""
    value, grad = _identity(*C.EDGES["wide-spread"])
    want = C.truth(*C.EDGES["wide-spread"], C.EDGE_CASE._replace(w_rank=0.0, w_recon=0.0, w_mse=0.0))
    assert abs(float(value - want.ple)) <= 1e-12 * abs(float(want.ple))
    assert float((grad - want.grad).abs().max()) <= 1e-12 * float(want.grad.abs().max())


# ---- the gates
@functools.lru_cache(maxsize=None)
def _errors(c):
    want, got = C.case_truth(c), C.case_truth(c, torch.float32)
    ev = max([C.rel_value(got.objective, want.objective)] + [C.rel_value(getattr(got, f), getattr(want, f)) for f in ("ple", "rank", "recon", "mse")])
    assert got.pairs == want.pairs
    return ev, C.rel_grad(got.grad, want.grad)


@functools.lru_cache(maxsize=None)
def _edge_errors(name, l2):
    want, got = C.edge_truth(name, l2), C.edge_truth(name, l2, torch.float32)
    ev = max([C.rel_value(got.objective, want.objective)] + [C.rel_value(getattr(got, f), getattr(want, f)) for f in ("ple", "rank", "recon", "mse")])
    return ev, C.rel_grad(got.grad, want.grad)


@pytest.mark.parametrize("c", _ALL, ids=C.ids(_ALL))
def test_fp32_restatement_stays_within_an_eighth_of_the_gates(c):
    ev, eg = _errors(c)
    assert ev <= C.VALUE_RTOL / 8 and eg <= C.GRAD_RTOL / 8


def _round_up_one_digit(v):
    m = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / m - 1e-9) * m


def test_gates_are_eight_times_the_fp32_restatement():
    """the gates of cox_cases.py are 8 x the worst figure over every case (tables, fixtures, edges), rounded up to one significant digit
    -- no tighter (a correct fp32 kernel reaches them) and no looser"""
    worst = {"value": (-1.0, ""), "gradient": (-1.0, "")}
    for c in _ALL:
        ev, eg = _errors(c)
        worst["value"] = max(worst["value"], (ev, c.name))
        worst["gradient"] = max(worst["gradient"], (eg, c.name))
    for name in C.EDGES:
        for l2 in (False, True):
            ev, eg = _edge_errors(name, l2)
            worst["value"] = max(worst["value"], (ev, name))
            worst["gradient"] = max(worst["gradient"], (eg, name))
    for kind, (err, where) in worst.items():
        print(f"worst fp32 restatement error, {kind}: {err:.3e} at {where} -> gate {_round_up_one_digit(8 * err):g}")
    assert math.isclose(C.VALUE_RTOL, _round_up_one_digit(8 * worst["value"][0]), rel_tol=1e-9)
    assert math.isclose(C.GRAD_RTOL, _round_up_one_digit(8 * worst["gradient"][0]), rel_tol=1e-9)


# ---- the Python layer, without a GPU
def test_from_handler_accepts_and_refuses_as_stated():
    from vlsa_amd import SurvPLE, SurvPairObjective, _native as nat, losses as L

    class _RefSurvPLE:                      # stands in for the reference's class: no options to read
        CONSTANT = torch.tensor(10.0)

    partials = {"rank_loss": functools.partial(L.rank_loss, gamma=2, norm="l2"), "recon_loss": functools.partial(L.recon_loss, alpha=0.3, gamma=0.5),
                "MSE_loss": functools.partial(L.MSE_loss, include_censored=True)}
    o = SurvPairObjective.from_handler(partials, {"rank_loss": 0.5, "recon_loss": 2.0, "MSE_loss": 1.0}, None)
    assert o._spec == (0.0, 0.5, 2.0, 1.0, 2.0, nat.PAIR_NORM_L2, 0.3, 0.5, nat.PAIR_NORM_L1, 1)
    for ple in (SurvPLE(), _RefSurvPLE()):
        o = SurvPairObjective.from_handler({"SurvPLE": ple}, {"SurvPLE": 1.0}, None)
        assert o._spec == (1.0, 0.0, 0.0, 0.0, 1.0, nat.PAIR_NORM_L1, 0.0, 1.0, nat.PAIR_NORM_L1, 0)
    assert o._spec == SurvPairObjective(weight_ple=1)._spec and o.weights["SurvPLE"] == 1.0
    plain = SurvPairObjective.from_handler({"rank_loss": L.rank_loss}, {"rank_loss": 1.0}, None)         # a plain function: its defaults
    assert plain._spec[:6] == (0.0, 1.0, 0.0, 0.0, 1.0, nat.PAIR_NORM_L1)
    for conv in ("softmax", "sigmoid"):
        with pytest.raises(ValueError, match="None"):                   # the handler's own check
            SurvPairObjective.from_handler({"SurvPLE": SurvPLE()}, {"SurvPLE": 1.0}, conv)
    with pytest.raises(NotImplementedError):
        SurvPairObjective.from_handler({"SurvMLE": object()}, {"SurvMLE": 1.0}, None)
    with pytest.raises(NotImplementedError, match="add_weight"):
        SurvPairObjective.from_handler({"rank_loss": functools.partial(L.rank_loss, add_weight=True)}, {"rank_loss": 1.0}, None)
    with pytest.raises(NotImplementedError):
        SurvPairObjective.from_handler({"rank_loss": functools.partial(L.rank_loss, norm="l3")}, {"rank_loss": 1.0}, None)
    with pytest.raises(NotImplementedError, match="add_weight"):
        L.rank_loss(torch.zeros(2), torch.zeros(2), torch.zeros(2), add_weight=True)


def test_modules_keep_the_references_signatures():
    import inspect
    from vlsa_amd import losses as L
    assert list(inspect.signature(L.recon_loss).parameters) == ["pred_t", "t", "e", "alpha", "gamma", "norm", "cur_alpha", "kws"]
    assert list(inspect.signature(L.rank_loss).parameters) == ["pred_t", "t", "e", "gamma", "norm", "add_weight", "kws"]
    assert list(inspect.signature(L.MSE_loss).parameters) == ["pred_t", "t", "e", "include_censored", "kws"]
    assert list(inspect.signature(L.SurvPLE.forward).parameters) == ["self", "y_hat", "T", "E"]
    assert float(L.SurvPLE(anything=1).CONSTANT) == C.CAP
    d = {n: inspect.signature(getattr(L, n)).parameters for n in ("recon_loss", "rank_loss", "MSE_loss")}
    assert (d["recon_loss"]["alpha"].default, d["recon_loss"]["gamma"].default, d["recon_loss"]["norm"].default) == (0.0, 1.0, "l1")
    assert (d["rank_loss"]["gamma"].default, d["rank_loss"]["norm"].default, d["rank_loss"]["add_weight"].default) == (1, "l1", False)
    assert d["MSE_loss"]["include_censored"].default is False
    assert "-0." in L.SurvPLE.__doc__ and "Tensor([0.])" in L.rank_loss.__doc__      # the stated differences from the reference


def test_cpu_tensors_and_other_shapes_are_refused():
    from vlsa_amd import SurvPLE, SurvPairObjective, VlsaNativeError, losses as L
    p, t, e = torch.zeros(3), torch.arange(3.0), torch.ones(3)
    for call in (lambda: SurvPLE()(p, t, e), lambda: L.rank_loss(p, t, e), lambda: L.recon_loss(p, t, e), lambda: L.MSE_loss(p, t, e),
                 lambda: SurvPairObjective(weight_ple=1)(p, torch.stack([t, e], dim=1)),
                 lambda: SurvPairObjective(weight_mse=1).value_and_grad(p.view(3, 1), t, e)):
        with pytest.raises(VlsaNativeError):
            call()


# ---- the binding: typed by hand from the declaration in include/vlsa_hip.h
V, I, D = c_void_p, c_int, c_double


def test_derived_signature_and_constants_equal_the_headers():
    from vlsa_amd import _native as nat
    assert nat._SIGNATURES["vlsa_surv_pair_objective"] == (I, [V, V, I, V, I, D, D, D, D, D, I, D, D, I, I, V, V, V])
    assert "vlsa_surv_pair_objective" in nat.exported_symbols() and nat.ABI_VERSION == 1
    header = open(os.path.join(REPO, "include", "vlsa_hip.h")).read()
    found = dict(re.findall(r"#define VLSA_(PAIR_\w+) (\d+)", header))
    assert len(found) == 12 and all(getattr(nat, k) == int(v) for k, v in found.items())
    assert (nat.PAIR_TIME_F32, nat.PAIR_TIME_F64, nat.PAIR_NORM_L1, nat.PAIR_NORM_L2, nat.PAIR_MAX_B) == (0, 1, 1, 2, 4096)
    assert (nat.PAIR_OBJ_TOTAL, nat.PAIR_OBJ_PLE, nat.PAIR_OBJ_RANK, nat.PAIR_OBJ_RECON, nat.PAIR_OBJ_MSE, nat.PAIR_OBJ_PAIRS,
            nat.PAIR_OBJ_WORDS) == (0, 1, 2, 3, 4, 5, 6)
    assert "OUT OF CONTRACT" in header                                  # labels other than 0 / 1


# ---- a split: the restatements the GPU evaluators are compared with, against the reference's own float64 results
_SPLITS = [(M, times) for M in C.SPLIT_SHAPES for times in C.TIMES]


def test_split_constants_match_the_source_and_the_header():
    from vlsa_amd import _native as nat
    src = open(os.path.join(REPO, "vlsa_amd", "csrc", "surv_pairs.hip")).read()
    assert C.SPLIT_TILE == int(re.search(r"\bkSplitTile = (\d+)\b", src).group(1))
    assert set(C.SPLIT_EDGES) >= {C.SPLIT_TILE - 1, C.SPLIT_TILE, C.SPLIT_TILE + 1} and max(C.SPLIT_SHAPES) == 1025
    header = open(os.path.join(REPO, "include", "vlsa_hip.h")).read()
    found = dict(re.findall(r"#define VLSA_((?:CEVAL|REVAL)_\w+) (\d+)", header))
    assert len(found) == 7 + 16 and all(getattr(nat, k) == int(v) for k, v in found.items())
    assert (nat.CEVAL_SUM_PLE, nat.CEVAL_EVENTS, nat.CEVAL_NONFINITE, nat.CEVAL_M, nat.CEVAL_CONCORDANT, nat.CEVAL_RESULT_WORDS) == (0, 1, 2, 3, 8, 16)
    assert nat.CEVAL_CONCORDANT == nat.EVAL_CONCORDANT and nat.CEVAL_COMPARABLE == nat.EVAL_COMPARABLE == nat.REVAL_COMPARABLE
    assert nat.REVAL_RESULT_WORDS == 18 and nat.REVAL_M == 17
    assert nat._SIGNATURES["vlsa_cox_risk_sets"] == (I, [V, V, V, I, D, V, V])
    assert nat._SIGNATURES["vlsa_cox_cum_hazard"] == (I, [V, V, V, I, V, I, V, V])
    assert nat._SIGNATURES["vlsa_cox_finish"] == (I, [V, V, V, I, D, V, V])
    assert nat._SIGNATURES["vlsa_reg_eval"] == (I, [V, V, V, I, D, I, D, D, I, D, V, V, V, V])


@pytest.mark.parametrize("M,times", _SPLITS, ids=[f"m{M}-{t}" for M, t in _SPLITS])
def test_split_restatements_reproduce_the_references_float64_results(M, times):
    import surv_eval_helpers as H
    fx, i = C.load_split_fixture(M, times), C.split_inputs(M, times)
    for k in ("y_hat", "reg_pred", "t", "e"):
        assert torch.equal(torch.from_numpy(fx[k]), getattr(i, k))
    for key, pred in (("cox", i.y_hat), ("reg", i.reg_pred)):
        counts = H.pair_counts(i.t.numpy(), i.e.numpy(), -pred.double().numpy())
        assert list(counts[:4]) == fx[key + "_counts"].tolist()                # counts exact
        assert abs(H.cindex(counts) - float(fx[key + "_cindex"])) <= 1e-12
    ple = C.ple_value(i.y_hat.double(), i.t.double(), i.e.double())
    assert abs(float(ple) - float(fx["loss_ple"])) <= 1e-12 * max(1.0, abs(float(fx["loss_ple"])))
    # Breslow: the reference's own order of operations reproduces its numbers to 1e-12; the identity (one sum per risk set, what the
    # kernels compute) lies within what the reference's running subtraction loses -- a bound worked out in breslow_by_subtraction
    times_u, Hs, bound = C.breslow_by_subtraction(i.y_hat, i.t, i.e)
    ref = torch.from_numpy(fx["cum_hazard"])
    assert torch.equal(times_u, torch.from_numpy(fx["time_points"]))
    assert float((Hs - ref).abs().max()) <= 1e-12
    rows = torch.from_numpy(fx["survival_rows"])
    assert float((C.survival_curves(i.y_hat, Hs)[rows] - torch.from_numpy(fx["survival_hat_rows"])).abs().max()) <= 1e-12
    times_i, Hc = C.breslow(i.y_hat, i.t, i.e)
    assert torch.equal(times_i, times_u)
    excess = ((Hc - ref).abs() - bound - 1e-12).max()
    print(f"m{M}-{times}: identity vs reference max |dH| {float((Hc - ref).abs().max()):.2e}, largest bound {float(bound.max()):.2e}")
    assert float(excess) <= 0.0
    assert float((Hc - ref).abs().max()) <= 1e-10                              # the bound the GPU tests apply, absolute
    got, pairs = C.reg_metrics(i.reg_pred, i.t, i.e)
    assert pairs == int(fx["reg_rank_pairs"])
    for k in C.REG_METRICS:
        want = float(fx["reg_" + k])
        assert (math.isnan(want) and math.isnan(got[k])) or abs(got[k] - want) <= 1e-12 * max(1.0, abs(want)), (k, got[k], want)


def test_evaluators_construct_and_refuse_without_a_gpu():
    from vlsa_amd import CoxSurvEvaluator, RegSurvEvaluator, VlsaNativeError
    assert CoxSurvEvaluator.valid_metrics == ["c_index", "loss", "loss_ple"]
    assert RegSurvEvaluator.valid_metrics == ["c_index", "loss", "loss_rank", "loss_recon", "loss_recon_org", "event_t_rae", "nonevent_t_rae",
                                              "event_t_nre", "nonevent_t_nre"]
    with pytest.raises(NotImplementedError):
        CoxSurvEvaluator(backend="SurvivalEVAL")
    with pytest.raises(KeyError):
        RegSurvEvaluator()
    with pytest.raises(RuntimeError, match="fit_baseline"):
        CoxSurvEvaluator().survival(torch.zeros(3))
    data = {"y": torch.tensor([[1.0, 1.0], [2.0, 0.0]]), "y_hat": torch.zeros(2, 1), "uid": None, "name": "test"}
    with pytest.raises(VlsaNativeError):
        CoxSurvEvaluator().compute(data, ["loss"])
    with pytest.raises(VlsaNativeError):
        RegSurvEvaluator(end_time=12.0).compute(data, ["loss"])
    with pytest.raises(AssertionError):
        CoxSurvEvaluator().compute(data, ["IBS"])
