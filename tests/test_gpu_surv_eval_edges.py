"""The launch shapes of vlsa_amd/csrc/surv_eval.hip that the fixtures (K <= 12, M <= 1025) do not reach: the rows kernel's workgroup
widths -- 256 threads up to K = 30, 192 for 31 .. 40, 128 for 41 .. 60, 64 for 61 .. 64, with the cross-wave reduction over 4, 3, 2 and
1 waves -- the pair kernel's j-ranges of more than one tile (M > 8192), the ext-loss variants, and labels outside [0, K).  The truth
is tests/surv_eval_helpers.py (float64, pinned to the reference's results by tests/test_surv_eval_cpu.py); gates as in
tests/test_gpu_surv_eval.py: counts exact, losses 1e-10 relative."""
import numpy as np
import pytest
import torch

import surv_eval_helpers as H
from test_gpu_surv_eval import DEV, LOSS_RTOL

pytestmark = pytest.mark.gpu

LS = 56.3
EXT = dict(logit_scale=LS, w_ifmle=0.7, w_emd=1.3, alpha=0.2, eps=1e-7, p=2, raw_distance=True)


def _draw(M, K, seed):
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn(M, K, generator=g) * 2.0
    t = torch.randint(0, K, (M,), generator=g)
    e = (torch.rand(M, generator=g) < 0.55).float()
    t[0], e[0], t[-1], e[-1] = 0, 1.0, K - 1, 1.0
    return raw, t, e


def _y(t, e):
    return torch.stack([t.double(), e.double()], dim=1).to(DEV)


def _no_pair_hangs_on_rounding(est, tied_tol=1e-8):
    d = np.abs(est[:, None] - est[None, :])[np.triu_indices(len(est), 1)]
    assert not np.any((d < 1e-12) | (np.abs(d - tied_tol) < 1e-12)), "a pair of this draw is decided by rounding: pick another seed"


def _ext_call():
    losses = {"SurvIFMLE": H.ExtLoss(alpha=EXT["alpha"], eps=EXT["eps"]), "SurvEMD": H.ExtLoss(p=EXT["p"], raw_distance=EXT["raw_distance"])}
    return losses, dict(loss_weight={"SurvIFMLE": EXT["w_ifmle"], "SurvEMD": EXT["w_emd"]}, logit_scale=LS)


# ---- 1. workgroup widths (M = 257 leaves a one-sample last chunk at 256, 192 (= 65th of 192), 128 and 64 threads)
@pytest.mark.parametrize("M", [63, 257])
@pytest.mark.parametrize("ptype", ["incidence", "hazard"])
@pytest.mark.parametrize("K", [30, 31, 40, 41, 60, 61, 64])
def test_every_workgroup_width_of_the_rows_kernel(K, ptype, M):
    from vlsa_amd import SurvEvaluator
    raw, t, e = _draw(M, K, 8000 + 100 * K + M)
    ext = EXT if ptype == "incidence" else None
    want = H.evaluate(raw.numpy(), t.numpy(), e.numpy(), ptype, ext=ext)
    _no_pair_hangs_on_rounding(want["est"])
    losses, kws = _ext_call() if ext else (None, {})
    ev = SurvEvaluator(ptype)
    out = ev.compute({"y": _y(t, e), "raw_y_hat": raw.to(DEV), "uid": None}, H.METRICS, kws_ext_loss=losses, ret_risk=True, ret_survival=True, **kws)
    assert [ev.counts[k] for k in H.COUNT_NAMES] == list(want["counts"])
    assert out["c_index"] == want["c_index"]
    keys = ["loss", "loss_mle", "loss_mle_org"] + (["loss_SurvIFMLE", "loss_SurvEMD"] if ext else [])
    assert set(out) == set(keys) | {"c_index", "risk", "survival_hat"}
    for k in keys:
        print(f"K={K} {ptype} M={M} {k}: got {out[k]!r} truth {want[k]!r} rel {abs(out[k] - want[k]) / abs(want[k]):.2e} (gate {LOSS_RTOL:g})")
        assert abs(out[k] - want[k]) <= LOSS_RTOL * abs(want[k]), k
    risk_tol = 4 * K * K * 2.0 ** -53                       # K sums of K terms, each at most 1
    risk_err = float(np.abs(out["risk"].cpu().numpy() - want["est"]).max())
    surv = H.survival(H.convert(raw, ptype), ptype).clamp(min=0).float()
    surv_err = float((out["survival_hat"].cpu() - surv).abs().max())
    print(f"K={K} {ptype} M={M}: risk {risk_err:.2e} (gate {risk_tol:.2e}) curves {surv_err:.2e} (gate 1e-07)")
    assert out["risk"].dtype == torch.float64 and out["risk"].shape == (M,) and risk_err <= risk_tol
    assert out["survival_hat"].dtype == torch.float32 and out["survival_hat"].shape == (M, K) and surv_err <= 1e-7


def test_converted_predictions_at_a_two_wave_workgroup():
    from vlsa_amd import SurvEvaluator
    M, K = 257, 41
    raw, t, e = _draw(M, K, 8900)
    y_hat = torch.softmax(raw, dim=-1)                      # an fp32 'y_hat' as the handler collects it
    est = H.estimate(y_hat.double(), "incidence").numpy()
    _no_pair_hangs_on_rounding(est)
    counts = H.pair_counts(t.numpy(), e.numpy(), est)
    ev = SurvEvaluator("incidence")
    out = ev.compute({"y": _y(t, e), "y_hat": y_hat.to(DEV)}, ["c_index", "loss_mle"], ret_risk=True)
    assert [ev.counts[k] for k in H.COUNT_NAMES] == list(counts) and out["c_index"] == H.cindex(counts)
    ref = H.loss_mle(y_hat.double(), t, e, "incidence")
    assert abs(out["loss_mle"] - ref) <= LOSS_RTOL * abs(ref)
    assert float(np.abs(out["risk"].cpu().numpy() - est).max()) <= 4 * K * K * 2.0 ** -53


# ---- 2. j-ranges of more than one tile: 8192 = 32 tiles, one per workgroup row; 8193 = 33 tiles, two per row, the 17th row holding
# one tile of one sample; 16385 = 65 tiles, three per row, the 22nd row two (one of them one sample)
@pytest.mark.parametrize("M", [8192, 8193, 16385])
def test_heavy_ties_across_the_j_ranges(M):
    from vlsa_amd import concordance_counts
    g = np.random.default_rng(200 + M)
    event = g.random(M) < 0.6
    event[0] = event[-1] = True                             # (the one sample of the last tile acts as an i, too)
    time = g.integers(0, 6, M).astype(np.float64)
    time[0], time[-1] = 0.0, 3.0
    est = g.choice(np.linspace(-1.0, 1.0, 8), M)
    want = H.pair_counts_blocked(time, event, est, rows=256)
    dev = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).to(DEV)      # noqa: E731
    got = concordance_counts(dev(time, torch.float64), dev(event, torch.float32), dev(est, torch.float64), 1e-8).tolist()
    print(f"M={M}: counts {got} truth {list(want)}")
    assert want[2] > 0 and want[3] > 0
    assert got == list(want)


# ---- 3. ext-loss variants
@pytest.mark.parametrize("name,losses", [
    ("emd_p1", {"SurvEMD": dict(p=1, raw_distance=True)}),
    ("emd_root", {"SurvEMD": dict(p=2, raw_distance=False)}),
    ("ifmle_alone", {"SurvIFMLE": dict(alpha=0.2, eps=1e-7)}),
    ("emd_alone", {"SurvEMD": dict(p=2, raw_distance=True)}),
    ("both_p1", {"SurvIFMLE": dict(alpha=0.0, eps=1e-7), "SurvEMD": dict(p=1, raw_distance=True)}),
])
def test_ext_loss_variants(name, losses):
    from vlsa_amd import SurvEvaluator
    fx = H.load_fixture("m65_k4_incidence")
    assert fx["raw"].shape == (65, 4)
    emd, ifmle = losses.get("SurvEMD", dict(p=2, raw_distance=True)), losses.get("SurvIFMLE", dict(alpha=0.0, eps=1e-7))
    ext = dict(logit_scale=LS, w_ifmle=0.7, w_emd=1.3, **emd, **ifmle)
    data = {"y": _y(torch.from_numpy(fx["t"]), torch.from_numpy(fx["e"])), "raw_y_hat": torch.from_numpy(fx["raw"]).to(DEV), "uid": None}
    out = SurvEvaluator("incidence").compute(data, ["loss"], kws_ext_loss={k: H.ExtLoss(**v) for k, v in losses.items()},
                                             loss_weight={"SurvIFMLE": 0.7, "SurvEMD": 1.3}, logit_scale=torch.tensor(LS, device=DEV))
    assert list(out) == ["loss"] + ["loss_" + k for k in losses]
    ls32 = float(torch.tensor(LS))                          # (the scale reaches the kernel as an fp32 tensor here)
    want = H.evaluate(fx["raw"], fx["t"], fx["e"], "incidence", ext=dict(ext, logit_scale=ls32))
    for k in out:
        print(f"{name} {k}: got {out[k]!r} truth {want[k]!r} rel {abs(out[k] - want[k]) / abs(want[k]):.2e} (gate {LOSS_RTOL:g})")
        assert abs(out[k] - want[k]) <= LOSS_RTOL * abs(want[k]), k


# ---- 4. labels outside [0, K): the losses read the clamped bin, the pair counts the raw time
@pytest.mark.parametrize("ptype", ["incidence", "hazard"])
def test_labels_out_of_range_are_clamped_for_the_losses_only(ptype):
    from vlsa_amd import SurvEvaluator
    from vlsa_amd import _native as nat
    M, K = 65, 4
    raw, t, e = _draw(M, K, 8800)
    idx = torch.arange(M)
    t_out = torch.where(idx % 4 == 1, torch.full_like(t, -1), torch.where(idx % 4 == 2, torch.full_like(t, K + 2), t))
    t_in = t_out.clamp(0, K - 1)
    losses, kws = _ext_call() if ptype == "incidence" else (None, {})
    ev = SurvEvaluator(ptype)
    words = slice(0, nat.EVAL_M + 1)
    res = [ev.compute_device({"y": _y(tt, e), "raw_y_hat": raw.to(DEV)}, ["loss", "loss_mle", "loss_mle_org"], kws_ext_loss=losses, **kws)
           for tt in (t_out, t_in)]
    assert torch.equal(res[0][words].view(torch.int64), res[1][words].view(torch.int64))
    ev.compute({"y": _y(t_out, e), "raw_y_hat": raw.to(DEV)}, ["c_index"])
    est = H.estimate(H.convert(raw, ptype), ptype).numpy()
    _no_pair_hangs_on_rounding(est)
    raw_counts, clamped_counts = H.pair_counts(t_out.numpy(), e.numpy(), est), H.pair_counts(t_in.numpy(), e.numpy(), est)
    assert raw_counts != clamped_counts
    assert [ev.counts[k] for k in H.COUNT_NAMES] == list(raw_counts)
