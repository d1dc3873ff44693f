"""CPU side of the device survival evaluator (vlsa_amd.evaluate): the float64 restatement the GPU tests use as their truth is pinned to
the reference's own float64 results (tests/golden/surv_eval_*.npz, written by tests/golden/make_golden_surv_eval.py), the fixtures keep
the conditions that make their pair counts independent of rounding, and the host-side refusals need no GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import surv_eval_helpers as H

NAMES = H.fixture_names()
SHAPES = {"m2_k2": (2, 2), "m3_k4": (3, 4), "m65_k4": (65, 4), "m257_k12": (257, 12), "m1025_k4": (1025, 4)}


def test_every_case_of_both_types_has_a_fixture():
    assert NAMES == sorted([f"{s}_{p}" for s in SHAPES for p in ("incidence", "hazard")] + ["lastbin_incidence"])
    for name in NAMES:
        fx = H.load_fixture(name)
        if name != "lastbin_incidence":
            assert fx["raw"].shape == SHAPES[name.rsplit("_", 1)[0]] and fx["raw"].dtype == np.float32
        assert str(fx["prediction_type"]) == name.rsplit("_", 1)[1]
        assert fx["t"].dtype == np.int64 and fx["e"].dtype == np.float32


@pytest.mark.parametrize("name", NAMES)
def test_helper_restates_the_reference_fed_float64(name):
    fx = H.load_fixture(name)
    ptype = str(fx["prediction_type"])
    got = H.evaluate(fx["raw"], fx["t"], fx["e"], ptype, ext=H.fixture_ext(fx))
    np.testing.assert_allclose(got["est"], fx["ref64_est"], rtol=0, atol=1e-12)
    keys = [k[len("ref64_"):] for k in fx if k.startswith("ref64_loss")]
    assert "loss" in keys and "loss_mle" in keys and "loss_mle_org" in keys
    assert (ptype == "incidence" and name != "lastbin_incidence") == ("loss_SurvEMD" in keys and "loss_SurvIFMLE" in keys)
    for k in keys:
        assert abs(got[k] - float(fx["ref64_" + k])) <= 1e-12, (k, got[k], float(fx["ref64_" + k]))
    if name == "lastbin_incidence":
        assert "ref64_counts" not in fx
        return
    assert list(got["counts"]) == fx["ref64_counts"].tolist()
    assert abs(got["c_index"] - float(fx["ref64_c_index"])) <= 1e-12
    assert float(fx["ref64_c_index"]) == float(fx["ref64_cindex_censored"])
    # (for information: the reference's plain fp32 run ranks these fixtures the same way)
    assert fx["ref32_counts"].tolist() == fx["ref64_counts"].tolist()


@pytest.mark.parametrize("name", [n for n in NAMES if n != "lastbin_incidence"])
def test_fixture_pair_counts_cannot_hang_on_rounding(name):
    fx = H.load_fixture(name)
    gaps = np.diff(np.sort(fx["ref64_est"]))
    assert np.all((gaps == 0) | (gaps >= H.MIN_RISK_GAP)), gaps[(gaps > 0) & (gaps < H.MIN_RISK_GAP)]
    # exact ties come only from bit-identical logit rows
    order = np.argsort(fx["ref64_est"], kind="stable")
    for a, b in zip(order[:-1], order[1:]):
        if fx["ref64_est"][a] == fx["ref64_est"][b]:
            assert np.array_equal(fx["raw"][a], fx["raw"][b])
    K = fx["raw"].shape[1]
    assert not np.any((fx["e"] == 0) & (fx["t"] == K - 1)), "a censored sample in the last bin"


def test_fixtures_carry_the_edge_cases():
    fxs = {n: H.load_fixture(n) for n in NAMES if n != "lastbin_incidence"}
    assert sum(int(f["ref64_counts"][2]) > 0 for f in fxs.values()) >= 4            # exact risk ties among comparable pairs
    assert sum(int(f["ref64_counts"][3]) > 0 for f in fxs.values()) >= 6            # tied times with mixed events
    assert any(bool(np.all(f["e"] == 1)) for f in fxs.values())                     # all events
    assert any(int(np.sum(f["e"])) == 1 and len(f["e"]) > 2 for f in fxs.values())  # one event


def test_censored_samples_in_the_last_bin_sit_on_the_clamp():
    fx = H.load_fixture("lastbin_incidence")
    assert np.all(fx["e"] == 0) and np.all(fx["t"] == fx["raw"].shape[1] - 1)
    lo = -math.log(1e-7)
    for v in (float(fx["ref64_loss_mle"]), H.evaluate(fx["raw"], fx["t"], fx["e"], "incidence")["loss_mle"]):
        assert lo <= v <= lo + 1e-6, v


def test_helper_pair_counts_on_a_case_done_by_hand():
    # times 1 1 2 3, events 1 0 1 0: i = 0 is comparable with 1 (same time, censored), 2, 3; i = 2 with 3
    time, event, est = [1.0, 1.0, 2.0, 3.0], [1, 0, 1, 0], [0.5, 0.5 + 5e-9, 0.5 + 2e-8, 0.1]
    # i = 0: j = 1 tied (5e-9 <= 1e-8), j = 2 discordant (larger estimate), j = 3 concordant; i = 2: j = 3 concordant
    assert H.pair_counts(time, event, est) == (2, 1, 1, 1, 4)
    assert H.cindex((2, 1, 1, 1, 4)) == 2.5 / 4


# ---- the Python surface: construction, refusals ----
def test_evaluator_construction_and_valid_metrics():
    from vlsa_amd import SurvEvaluator, evaluate
    assert SurvEvaluator is evaluate.SurvEvaluator
    for ptype in ("incidence", "hazard"):
        ev = SurvEvaluator(ptype)
        assert ev.type == ptype and ev.valid_metrics == ["c_index", "loss", "loss_mle", "loss_mle_org"]
        assert (ev.alpha, ev.eps, ev.tied_tol) == (0.0, 1e-7, 1e-8)
    with pytest.raises(AssertionError):
        SurvEvaluator("hazard_ratio")
    with pytest.raises(NotImplementedError):
        SurvEvaluator("incidence", backend="SurvivalEVAL")
    with pytest.raises(AssertionError):
        SurvEvaluator("incidence").compute({"y": torch.zeros(2, 2), "y_hat": torch.zeros(2, 2)}, ["IBS"])


@pytest.mark.parametrize("losses,ptype", [
    ({"SurvEMD": H.ExtLoss(p=3, raw_distance=True)}, "incidence"),
    ({"SurvEMD": H.ExtLoss(p=2, raw_distance=True, reduction="sum")}, "incidence"),
    ({"SurvIFMLE": H.ExtLoss(alpha=0.0, eps=1e-7, reduction="none")}, "incidence"),
    ({"SurvIFMLE": H.ExtLoss(alpha=0.0, eps=1e-7)}, "hazard"),
])
def test_ext_losses_outside_the_kernel_are_not_implemented(losses, ptype):
    from vlsa_amd import SurvEvaluator
    data = {"y": torch.tensor([[0.0, 1.0], [1.0, 0.0]]), "raw_y_hat": torch.zeros(2, 2)}
    with pytest.raises(NotImplementedError):       # (raised before a tensor is looked at)
        SurvEvaluator(ptype).compute(data, ["loss"], kws_ext_loss=losses)


def test_cpu_tensors_are_refused():
    from vlsa_amd import SurvEvaluator, VlsaNativeError, concordance_counts, concordance_index_censored
    data = {"y": torch.tensor([[0.0, 1.0], [1.0, 0.0]]), "raw_y_hat": torch.zeros(2, 2), "uid": None}
    with pytest.raises(VlsaNativeError):
        SurvEvaluator("incidence").compute(data, ["c_index", "loss"])
    with pytest.raises(VlsaNativeError):
        SurvEvaluator("hazard").compute_device(data, ["loss"])
    with pytest.raises(VlsaNativeError):
        concordance_index_censored(torch.tensor([True, False]), torch.tensor([1.0, 2.0]), torch.tensor([0.3, 0.1]))
    with pytest.raises(VlsaNativeError):
        concordance_counts(np.array([1.0, 2.0]), np.array([1, 0]), np.array([0.3, 0.1]))


# ---- the C entry points refuse bad arguments before anything is launched ----
def _rows(lib, x, t, e, M, K, est, time, result, x_kind=0, pred_type=0, ext_mask=0, p=2):
    return lib.vlsa_surv_eval_rows(x, x_kind, pred_type, t, e, M, K, 0.0, 1e-7, None, 10.0, 0, ext_mask, 0.0, 1e-7, p, 1, 1.0, 1.0,
                                   est, time, None, result, None)


def test_entry_points_refuse_bad_arguments():
    from vlsa_amd import _native as nat
    lib = nat.load()
    buf = (ctypes.c_double * 64)()                 # never read: every call below returns before a launch
    a = ctypes.addressof(buf)
    assert (nat.EVAL_MAX_M, nat.EVAL_RESULT_WORDS, nat.EVAL_CONCORDANT, nat.EVAL_COMPARABLE) == (65536, 16, 8, 12)
    for hole in range(6):                          # a NULL among x, t, e, est, time, result
        ptrs = [a] * 6
        ptrs[hole] = None
        x, t, e, est, time, result = ptrs
        assert _rows(lib, x, t, e, 4, 4, est, time, result) == nat.EINVAL, hole
    for M, K in [(0, 4), (-1, 4), (4, 0), (4, nat.MAX_K + 1), (70000, 0)]:
        assert _rows(lib, a, a, a, M, K, a, a, a) == nat.EINVAL, (M, K)
    assert _rows(lib, a, a, a, 4, 4, a, a, a, x_kind=2) == nat.EINVAL
    assert _rows(lib, a, a, a, 4, 4, a, a, a, pred_type=2) == nat.EINVAL
    assert _rows(lib, a, a, a, 4, 4, a, a, a, ext_mask=4) == nat.EINVAL
    assert _rows(lib, a, a, a, nat.EVAL_MAX_M + 1, 4, a, a, a) == nat.EUNSUPPORTED
    assert _rows(lib, a, a, a, 4, 4, a, a, a, pred_type=nat.EVAL_HAZARD, ext_mask=1) == nat.EUNSUPPORTED
    assert _rows(lib, a, a, a, 4, 4, a, a, a, ext_mask=2, p=3) == nat.EUNSUPPORTED
    for hole in range(4):                          # time, e, est, counters
        ptrs = [a] * 4
        ptrs[hole] = None
        assert lib.vlsa_concordance_pairs(ptrs[0], ptrs[1], ptrs[2], 4, 1e-8, ptrs[3], 0, None) == nat.EINVAL, hole
    assert lib.vlsa_concordance_pairs(a, a, a, 0, 1e-8, a, 0, None) == nat.EINVAL
    assert lib.vlsa_concordance_pairs(a, a, a, nat.EVAL_MAX_M + 1, 1e-8, a, 1, None) == nat.EUNSUPPORTED
