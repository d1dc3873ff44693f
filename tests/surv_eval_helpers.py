"""Float64 CPU restatement of what vlsa_amd.evaluate computes on the device (torch / numpy only, no reference import): the handler's
output converter, the risk Harrell's C ranks by (eval/cindex.py:36-43), the pair counts of the vendored scikit-survival
concordance_index_censored (eval/cindex.py:86-150, restated by its definition, vectorised over all pairs), SurvIFMLE / SurvMLE
(loss/loss_surv.py:104-169) and SurvEMD (loss/loss_surv_ext.py:13-109).  tests/test_surv_eval_cpu.py pins it to the reference's own
float64 results in tests/golden/surv_eval_*.npz; the GPU tests use it as the truth for inputs that have no fixture."""
import glob
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COUNT_NAMES = ("concordant", "discordant", "tied_risk", "tied_time", "comparable")
METRICS = ["c_index", "loss", "loss_mle", "loss_mle_org"]
MIN_RISK_GAP = 1e-6            # every non-zero gap between sorted fixture risks: 100 x tied_tol


def fixture_names():
    return sorted(os.path.basename(p)[len("surv_eval_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "surv_eval_*.npz")))


def load_fixture(name):
    with np.load(os.path.join(GOLDEN, f"surv_eval_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def convert(raw, prediction_type):
    raw = torch.as_tensor(raw).double()
    return torch.softmax(raw, dim=-1) if prediction_type == "incidence" else torch.sigmoid(raw)


def survival(y_hat, prediction_type):
    """the unclamped curve S [M, K] (float64)"""
    y_hat = torch.as_tensor(y_hat).double()
    return 1.0 - torch.cumsum(y_hat, dim=1) if prediction_type == "incidence" else torch.cumprod(1.0 - y_hat, dim=1)


def estimate(y_hat, prediction_type):
    """-sum_k S_k: the estimate handed to concordance_index_censored"""
    return -survival(y_hat, prediction_type).sum(dim=1)


def pair_counts(time, event, est, tied_tol=1e-8):
    """(concordant, discordant, tied_risk, tied_time, comparable) as Python ints"""
    time, est = np.asarray(time, dtype=np.float64), np.asarray(est, dtype=np.float64)
    event = np.asarray(event) != 0
    ti, tj = time[:, None], time[None, :]
    same = event[:, None] & (tj == ti) & ~event[None, :]
    comp = (event[:, None] & (tj > ti)) | same
    tied = np.abs(est[None, :] - est[:, None]) <= tied_tol
    con = comp & ~tied & (est[None, :] < est[:, None])
    n_comp, n_con, n_tied = int(comp.sum()), int(con.sum()), int((comp & tied).sum())
    return n_con, n_comp - n_con - n_tied, n_tied, int(same.sum()), n_comp


def pair_counts_blocked(time, event, est, tied_tol=1e-8, rows=512):
    """pair_counts, `rows` samples i at a time: the all-pairs matrices of M = 16 385 would take 2 GB"""
    time, est = np.asarray(time, dtype=np.float64), np.asarray(est, dtype=np.float64)
    event = np.asarray(event) != 0
    n_comp = n_con = n_tied = n_same = 0
    for i0 in range(0, len(time), rows):
        ev = event[i0:i0 + rows, None]
        ti, si = time[i0:i0 + rows, None], est[i0:i0 + rows, None]
        same = ev & (time[None, :] == ti) & ~event[None, :]
        comp = (ev & (time[None, :] > ti)) | same
        tied = np.abs(est[None, :] - si) <= tied_tol
        n_con += int((comp & ~tied & (est[None, :] < si)).sum())
        n_comp, n_tied, n_same = n_comp + int(comp.sum()), n_tied + int((comp & tied).sum()), n_same + int(same.sum())
    return n_con, n_comp - n_con - n_tied, n_tied, n_same, n_comp


def cindex(counts):
    con, _, tied, _, comp = counts
    return (float(con) + 0.5 * float(tied)) / float(comp)


def loss_mle(y_hat, t, e, prediction_type, alpha=0.0, eps=1e-7, reduce=True, dtype=torch.float64):
    """dtype: the precision the formulas are evaluated in (float64: the truth; float32: what a plain fp32 evaluation of them reaches)"""
    y_hat = torch.as_tensor(y_hat).to(dtype)
    M = y_hat.shape[0]
    t = torch.as_tensor(t).view(M, 1).long()
    c = 1.0 - torch.as_tensor(e).view(M, 1).to(dtype)
    if prediction_type == "incidence":
        unc = -(1 - c) * torch.log(torch.gather(y_hat, 1, t).clamp(min=eps))
        cen = -c * torch.log((1 - torch.gather(torch.cumsum(y_hat, dim=1), 1, t)).clamp(min=eps))
    else:
        S = torch.cat([torch.ones_like(c), torch.cumprod(1 - y_hat, dim=1)], 1)
        unc = -(1 - c) * (torch.log(torch.gather(S, 1, t).clamp(min=eps)) + torch.log(torch.gather(y_hat, 1, t).clamp(min=eps)))
        cen = -c * torch.log(torch.gather(S, 1, t + 1).clamp(min=eps))
    loss = (1.0 - alpha) * (cen + unc) + alpha * unc
    return float(loss.mean()) if reduce else loss.view(M)


def loss_emd(y_hat, t, e, logit_scale, p=2, raw_distance=True):
    y_hat = torch.as_tensor(y_hat).double()
    M, K = y_hat.shape
    ls = float(logit_scale)
    t = torch.as_tensor(t).view(M, 1).long()
    ei = torch.as_tensor(e).view(M, 1).long()
    k = torch.arange(K).view(1, K)
    target = ((k == t).long() + (k > t).long() * (1 - ei)).double()                 # convert_survival_label
    target_dist = torch.softmax((2 * target - 1) * ls, dim=-1)
    pred = (1 - ei) * ((1 - target) * y_hat + target * ls) + ei * y_hat
    d = torch.cumsum(torch.softmax(pred, dim=-1), dim=-1) - torch.cumsum(target_dist, dim=-1)
    dist = d.abs().sum(dim=-1) if p == 1 else (d ** 2).sum(dim=-1)
    if p == 2 and not raw_distance:
        dist = dist.sqrt()
    return float(dist.mean())


def loss_emd_rows(y_hat, t, e, logit_scale, p=2, raw_distance=True, dtype=torch.float64):
    """loss_emd per sample: the [M] tensor whose mean loss_emd returns, differentiable w.r.t. y_hat (dtype: as in loss_mle)"""
    y_hat = torch.as_tensor(y_hat).to(dtype)
    M, K = y_hat.shape
    ls = float(logit_scale)
    t = torch.as_tensor(t).view(M, 1).long()
    ei = torch.as_tensor(e).view(M, 1).long()
    k = torch.arange(K).view(1, K)
    target = ((k == t).long() + (k > t).long() * (1 - ei)).to(dtype)                # convert_survival_label
    target_dist = torch.softmax((2 * target - 1) * ls, dim=-1)
    pred = (1 - ei) * ((1 - target) * y_hat + target * ls) + ei * y_hat
    d = torch.cumsum(torch.softmax(pred, dim=-1), dim=-1) - torch.cumsum(target_dist, dim=-1)
    dist = d.abs().sum(dim=-1) if p == 1 else (d ** 2).sum(dim=-1)
    if p == 2 and not raw_distance:
        dist = dist.sqrt()
    return dist


def evaluate(raw, t, e, prediction_type, alpha=0.0, eps=1e-7, tied_tol=1e-8, ext=None):
    """every number of SurvEvaluator.compute from the raw logits: {'c_index', 'loss', 'loss_mle', 'loss_mle_org', 'counts', 'est'} and,
    with ext = dict(logit_scale, w_ifmle, w_emd, alpha, eps, p, raw_distance), 'loss_SurvIFMLE' / 'loss_SurvEMD'"""
    y_hat = convert(raw, prediction_type)
    est = estimate(y_hat, prediction_type)
    counts = pair_counts(np.asarray(t, dtype=np.float64), np.asarray(e), est.numpy(), tied_tol)
    out = dict(est=est.numpy(), counts=counts, c_index=cindex(counts) if counts[4] else float("nan"),
               loss_mle=loss_mle(y_hat, t, e, prediction_type, alpha, eps), loss_mle_org=loss_mle(y_hat, t, e, prediction_type, 0.0, eps))
    out["loss"] = out["loss_mle_org"]
    if ext is not None:
        out["loss_SurvIFMLE"] = ext["w_ifmle"] * loss_mle(y_hat, t, e, "incidence", ext["alpha"], ext["eps"])
        out["loss_SurvEMD"] = ext["w_emd"] * loss_emd(y_hat, t, e, ext["logit_scale"], ext["p"], ext["raw_distance"])
    return out


def fixture_ext(fx):
    """the ext-loss settings of a fixture, or None (hazard fixtures carry none)"""
    if "w_ifmle" not in fx:
        return None
    return dict(logit_scale=float(fx["logit_scale"]), w_ifmle=float(fx["w_ifmle"]), w_emd=float(fx["w_emd"]), alpha=float(fx["ext_alpha"]),
                eps=float(fx["ext_eps"]), p=int(fx["p"]), raw_distance=bool(fx["raw_distance"]))


class ExtLoss:
    """stands in for a SurvIFMLE / SurvEMD instance of either code base: SurvEvaluator reads the attributes only"""

    def __init__(self, **kw):
        self.reduction = "mean"
        self.__dict__.update(kw)


def fixture_call(fx):
    """(kws_ext_loss, kws) of SurvEvaluator.compute for a fixture"""
    ext = fixture_ext(fx)
    if ext is None:
        return None, {}
    losses = {"SurvIFMLE": ExtLoss(alpha=ext["alpha"], eps=ext["eps"]), "SurvEMD": ExtLoss(p=ext["p"], raw_distance=ext["raw_distance"])}
    return losses, dict(loss_weight={"SurvIFMLE": ext["w_ifmle"], "SurvEMD": ext["w_emd"]}, logit_scale=float(fx["logit_scale"]))
