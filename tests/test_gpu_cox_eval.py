"""The Cox and Reg evaluators on the device (vlsa_amd.evaluate.CoxSurvEvaluator / RegSurvEvaluator over the split launches of
vlsa_amd/csrc/surv_pairs.hip) against the reference's own float64 results (tests/golden/cox_split_*.npz, which
tests/test_cox_cases_cpu.py pins the restatements of tests/cox_cases.py to) and, past the launches' tile edge, against those restatements.
Float64 device work: counts exact, C within 1e-12, losses and metrics within 1e-10 of max(1, |value|) (the bounds
tests/test_gpu_surv_eval.py uses), H and the curves within 1e-10 absolute."""
import math

import pytest
import torch

import cox_cases as C
import surv_eval_helpers as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = 1e-10
_SPLITS = [(M, times) for M in C.SPLIT_SHAPES for times in C.TIMES]
_IDS = [f"m{M}-{t}" for M, t in _SPLITS]
COX_METRICS = ["c_index", "loss", "loss_ple"]


def _close(got, want, tol=TOL):
    return (math.isnan(want) and math.isnan(got)) or abs(got - want) <= tol * max(1.0, abs(want))


def _data(pred, t, e, name="test", column=True):
    y = torch.stack([t.double(), e.double()], dim=1).to(DEV)
    return {"y": y, "y_hat": (pred.view(-1, 1) if column else pred).to(DEV), "uid": None, "name": name}


# ---- 1. the fixtures
@pytest.mark.parametrize("M,times", _SPLITS, ids=_IDS)
def test_cox_evaluator_against_the_references_float64_results(M, times):
    from vlsa_amd import CoxSurvEvaluator
    fx, i = C.load_split_fixture(M, times), C.split_inputs(M, times)
    ev = CoxSurvEvaluator()
    got = ev.compute(_data(i.y_hat, i.t, i.e, "train"), COX_METRICS, ret_survival=True)
    assert list(got) == COX_METRICS + ["survival_hat", "time_points"]
    assert [ev.counts[k] for k in ("concordant", "discordant", "tied_risk", "tied_time")] == fx["cox_counts"].tolist()       # exact
    assert abs(got["c_index"] - float(fx["cox_cindex"])) <= 1e-12
    print(f"m{M}-{times}: loss_ple {got['loss_ple']:.12g} reference {float(fx['loss_ple']):.12g}")
    assert got["loss"] == got["loss_ple"] and _close(got["loss_ple"], float(fx["loss_ple"]))
    assert torch.equal(got["time_points"].cpu(), torch.from_numpy(fx["time_points"]))
    ref = torch.from_numpy(fx["cum_hazard"])
    err = float((ev.cum_hazard.cpu() - ref).abs().max())
    print(f"m{M}-{times}: max |H - reference| {err:.2e} of {float(ref.abs().max()):.3g}")
    assert ev.cum_hazard.dtype == torch.float64 and err <= TOL                 # absolute, as for the curves
    surv = got["survival_hat"]
    assert surv.shape == (M, len(fx["time_points"])) and surv.dtype == torch.float64
    rows = torch.from_numpy(fx["survival_rows"])
    assert float((surv.cpu()[rows] - torch.from_numpy(fx["survival_hat_rows"])).abs().max()) <= TOL


@pytest.mark.parametrize("M,times", _SPLITS, ids=_IDS)
def test_reg_evaluator_against_the_references_float64_results(M, times):
    from vlsa_amd import RegSurvEvaluator
    fx, i = C.load_split_fixture(M, times), C.split_inputs(M, times)
    ev = RegSurvEvaluator(end_time=float(fx["end_time"]))
    metrics = list(ev.valid_metrics)
    got = ev.compute(_data(i.reg_pred, i.t, i.e), metrics)
    assert list(got) == metrics and ev.rank_pairs == int(fx["reg_rank_pairs"])
    assert [ev.counts[k] for k in ("concordant", "discordant", "tied_risk", "tied_time")] == fx["reg_counts"].tolist()
    assert abs(got["c_index"] - float(fx["reg_cindex"])) <= 1e-12             # the call behind the reference's assertion, estimate -y_hat
    for k in C.REG_METRICS:
        print(f"m{M}-{times}: {k} {got[k]:.12g} reference {float(fx['reg_' + k]):.12g}")
        assert _close(got[k], float(fx["reg_" + k])), k


# ---- 2. past the tile edge of the split launches, and other options, against the float64 restatement
@pytest.mark.parametrize("times", C.TIMES)
@pytest.mark.parametrize("M", C.SPLIT_EDGES)
def test_evaluators_at_the_tile_edges(M, times):
    from vlsa_amd import CoxSurvEvaluator, RegSurvEvaluator
    i = C.split_inputs(M, times)
    cox = CoxSurvEvaluator()
    got = cox.compute(_data(i.y_hat, i.t, i.e, "train", column=False), COX_METRICS, ret_survival=True)
    counts = H.pair_counts(i.t.numpy(), i.e.numpy(), -i.y_hat.double().numpy())
    assert tuple(cox.counts.values()) == counts and abs(got["c_index"] - H.cindex(counts)) <= 1e-12
    assert _close(got["loss_ple"], float(C.ple_value(i.y_hat.double(), i.t.double(), i.e.double())))
    times_u, Hc = C.breslow(i.y_hat, i.t, i.e)
    assert torch.equal(got["time_points"].cpu(), times_u)
    assert float((cox.cum_hazard.cpu() - Hc).abs().max()) <= TOL
    assert float((got["survival_hat"].cpu() - C.survival_curves(i.y_hat, Hc)).abs().max()) <= TOL
    opts = dict(alpha=0.3, gamma=0.5, norm="l2", rank_gamma=0.5, rank_norm="l2")
    reg = RegSurvEvaluator(end_time=C.END_TIME, **opts)
    res = reg.compute(_data(i.reg_pred, i.t, i.e), list(C.REG_METRICS))
    want, pairs = C.reg_metrics(i.reg_pred, i.t, i.e, C.END_TIME, **opts)
    assert reg.rank_pairs == pairs
    for k in C.REG_METRICS:
        assert _close(res[k], want[k]), (k, res[k], want[k])
    assert res["loss_recon"] != res["loss_recon_org"]


# ---- 3. two runs, two routes
@pytest.mark.parametrize("M,times", [(257, "ties"), (1025, "f32")])
def test_two_runs_give_the_same_bits_and_read_equals_compute(M, times):
    from vlsa_amd import CoxSurvEvaluator, RegSurvEvaluator
    i = C.split_inputs(M, times)
    cox, reg = CoxSurvEvaluator(), RegSurvEvaluator(end_time=C.END_TIME)
    dc, dr = _data(i.y_hat, i.t, i.e), _data(i.reg_pred, i.t, i.e)
    a, b = cox.compute_device(dc, COX_METRICS), cox.compute_device(dc, COX_METRICS)
    assert a.shape == (16,) and torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert cox.read(a, COX_METRICS) == cox.compute(dc, COX_METRICS)
    rm = list(reg.valid_metrics)
    a, b = reg.compute_device(dr, rm), reg.compute_device(dr, rm)
    assert a.shape == (18,) and torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert reg.read(a, rm) == reg.compute(dr, rm)
    cox.fit_baseline(dc["y_hat"], i.t.to(DEV), i.e.to(DEV))
    h1 = cox.cum_hazard.clone()
    cox.fit_baseline(dc["y_hat"], i.t.to(DEV), i.e.to(DEV))
    assert torch.equal(h1.view(torch.int64), cox.cum_hazard.view(torch.int64))


def test_a_train_pass_fits_the_baseline_a_test_pass_reuses():
    from vlsa_amd import CoxSurvEvaluator
    tr, te = C.split_inputs(257, "f32"), C.split_inputs(65, "ties")
    ev = CoxSurvEvaluator()
    with pytest.raises(RuntimeError, match="fit_baseline"):                    # curves before a fit
        ev.compute(_data(te.y_hat, te.t, te.e, "test"), ["loss"], ret_survival=True)
    assert "survival_hat" not in ev.compute(_data(te.y_hat, te.t, te.e, "test"), ["loss"])      # the metrics alone need no baseline
    ev.compute(_data(tr.y_hat, tr.t, tr.e, "train"), ["loss"])
    times_u, Hc = C.breslow(tr.y_hat, tr.t, tr.e)
    fitted = ev.cum_hazard.clone()
    got = ev.compute(_data(te.y_hat, te.t, te.e, "test"), COX_METRICS, ret_survival=True)
    assert torch.equal(ev.cum_hazard, fitted) and torch.equal(got["time_points"].cpu(), times_u)       # the training split's baseline
    assert got["survival_hat"].shape == (65, 257)
    assert float((got["survival_hat"].cpu() - C.survival_curves(te.y_hat, Hc)).abs().max()) <= TOL
    assert _close(got["loss_ple"], float(C.ple_value(te.y_hat.double(), te.t.double(), te.e.double())))


# ---- 4. the reference's refusals arrive as ValueError after the copy
def test_refusals():
    from vlsa_amd import CoxSurvEvaluator, RegSurvEvaluator
    evs = [(CoxSurvEvaluator(), ["c_index"]), (RegSurvEvaluator(end_time=C.END_TIME), ["c_index"])]
    t, e = torch.tensor([1.0, 2.0, 3.0]), torch.tensor([1.0, 0.0, 1.0])
    for ev, m in evs:
        with pytest.raises(ValueError, match="minimum of two"):
            ev.compute(_data(torch.zeros(1), t[:1], e[:1]), m)
        with pytest.raises(ValueError, match="censored"):
            ev.compute(_data(torch.zeros(3), t, torch.zeros(3)), m)
        with pytest.raises(ValueError, match="comparable"):                     # the only event sits at the largest time
            ev.compute(_data(torch.zeros(3), t, torch.tensor([0.0, 0.0, 1.0])), m)
        for bad in (float("nan"), float("inf")):
            with pytest.raises(ValueError, match="NaN or infinity"):
                ev.compute(_data(torch.tensor([0.5, bad, 1.0]), t, e), m)
        with pytest.raises(ValueError, match="one-column"):
            ev.compute(dict(_data(torch.zeros(3), t, e), y_hat=torch.zeros(3, 2, device=DEV)), m)
    # the losses are computed where C is refused, as the reference computes them
    assert CoxSurvEvaluator().compute(_data(torch.zeros(3), t, torch.zeros(3)), ["loss"])["loss"] == 0.0
    res = RegSurvEvaluator(end_time=C.END_TIME).compute(_data(torch.zeros(3), t, torch.zeros(3)), ["event_t_rae", "nonevent_t_rae", "loss_rank"])
    assert math.isnan(res["event_t_rae"]) and _close(res["nonevent_t_rae"], 2.0 / C.END_TIME) and res["loss_rank"] == 0.0


def test_split_launches_refuse_bad_arguments_before_any_launch():
    from vlsa_amd import _native as nat
    from vlsa_amd.functional import _p, _stream
    lib = nat.load()
    M = 8
    th, t, e = torch.zeros(M, device=DEV), torch.arange(float(M), device=DEV, dtype=torch.float64), torch.ones(M, device=DEV)
    D = torch.full((M,), -7.0, dtype=torch.float64, device=DEV)
    out = torch.full((nat.REVAL_RESULT_WORDS + 2 * M,), -7.0, dtype=torch.float64, device=DEV)
    big = nat.EVAL_MAX_M + 1
    assert lib.vlsa_cox_risk_sets(None, _p(t), _p(e), M, 10.0, _p(D), _stream()) == nat.EINVAL
    assert lib.vlsa_cox_risk_sets(_p(th), _p(t), _p(e), 0, 10.0, _p(D), _stream()) == nat.EINVAL
    assert lib.vlsa_cox_risk_sets(_p(th), _p(t), _p(e), M, float("nan"), _p(D), _stream()) == nat.EINVAL
    assert lib.vlsa_cox_risk_sets(_p(th), _p(t), _p(e), big, 10.0, _p(D), _stream()) == nat.EUNSUPPORTED
    assert lib.vlsa_cox_cum_hazard(_p(t), _p(e), _p(D), M, _p(t), 0, _p(D), _stream()) == nat.EINVAL
    assert lib.vlsa_cox_cum_hazard(_p(t), _p(e), _p(D), M, _p(t), big, _p(D), _stream()) == nat.EUNSUPPORTED
    assert lib.vlsa_cox_finish(_p(th), _p(e), None, M, 10.0, _p(out), _stream()) == nat.EINVAL
    assert lib.vlsa_cox_finish(_p(th), _p(e), _p(D), big, 10.0, _p(out), _stream()) == nat.EUNSUPPORTED
    args = (1.0, nat.PAIR_NORM_L1, 0.0, 1.0, nat.PAIR_NORM_L1, 12.0)
    assert lib.vlsa_reg_eval(_p(th), _p(t), _p(e), M, 1.0, 0, 0.0, 1.0, nat.PAIR_NORM_L1, 12.0, _p(out[18:]), None, _p(out), _stream()) == nat.EINVAL
    assert lib.vlsa_reg_eval(_p(th), _p(t), _p(e), M, *args, None, None, _p(out), _stream()) == nat.EINVAL
    assert lib.vlsa_reg_eval(_p(th), _p(t), _p(e), big, *args, _p(out[18:]), None, _p(out), _stream()) == nat.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((D == -7.0).all()) and bool((out == -7.0).all())                # no kernel wrote
