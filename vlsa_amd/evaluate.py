"""Scoring a split on the device: the reference's ``NLLSurv_Evaluator`` (eval/evaluator_surv.py:45-235, a backend other than
SurvivalEVAL) and its vendored ``concordance_index_censored`` (eval/cindex.py:152-207) on the [M, K] logits and (t, e) labels that are
already in HBM after an evaluation pass.  Two launches -- ``vlsa_surv_eval_rows`` (per sample, float64: converter, survival curve,
risk, loss sums) and ``vlsa_concordance_pairs`` (every pair, integer counts) -- and ONE device-to-host copy of a 128-byte result
buffer; Harrell's C is formed on the host from the exact counts.  No CPU fallback: a CPU tensor raises ``VlsaNativeError``.

What stays on the host: the SurvivalEVAL metrics (C on the mean survival time, IBS, MAE, D-calibration), which go through splines and
Kaplan-Meier fits of the training set; ``compute(..., ret_survival=True)`` hands back the clamped survival curves for them.

``CoxSurvEvaluator`` and ``RegSurvEvaluator`` are the reference's ``Cox`` and ``Reg`` evaluators for a one-column prediction (the
launches of ``csrc/surv_pairs.hip``), with ``compute``, ``compute_device`` and ``read`` in the same manner.
"""
from __future__ import annotations

import torch

from . import _native as nat
from .bag_tables import _need_gpu, _p, _stream

_COUNTERS = slice(nat.EVAL_CONCORDANT, nat.EVAL_COMPARABLE + 1)
_TYPES = {"incidence": nat.EVAL_INCIDENCE, "hazard": nat.EVAL_HAZARD}


def _labels(t, e, M, device):
    t = t.reshape(-1).to(device=device, dtype=torch.int64).contiguous()
    e = e.reshape(-1).to(device=device, dtype=torch.float32).contiguous()
    if t.numel() != M or e.numel() != M:
        raise ValueError("t and e must hold one entry per sample")
    return t, e


def _as_tensor(v):
    return v if isinstance(v, torch.Tensor) else torch.as_tensor(v)


def concordance_counts(time, event, estimate, tied_tol=1e-8):
    """The pair counts of ``concordance_index_censored`` as a device tensor of five int64 (concordant, discordant, tied_risk,
    tied_time, comparable), without a synchronisation.  time / estimate: [M] of any real dtype (compared in float64), event: [M],
    non-zero = event; 1 <= M <= 65 536."""
    time, event, estimate = _as_tensor(time), _as_tensor(event), _as_tensor(estimate)
    _need_gpu(time, event, estimate)
    lib = nat.load()
    dev = estimate.device
    est = estimate.detach().reshape(-1).to(dtype=torch.float64).contiguous()
    M = est.numel()
    tm = time.detach().reshape(-1).to(device=dev, dtype=torch.float64).contiguous()
    ev = event.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
    if tm.numel() != M or ev.numel() != M:
        raise ValueError("time, event and estimate must hold one entry per sample")
    if M < 1:
        raise ValueError("Need a minimum of two samples")
    counters = torch.empty(5, dtype=torch.int64, device=dev)
    nat.check(lib.vlsa_concordance_pairs(_p(tm), _p(ev), _p(est), M, float(tied_tol), _p(counters), 1, _stream()), "vlsa_concordance_pairs")
    return counters


def _cindex(concordant, discordant, tied_risk, tied_time, comparable):
    """(cindex, concordant, discordant, tied_risk, tied_time) from the counts: the reference's ``numerator / denominator`` with unit
    weights (eval/cindex.py:142-149), in float64.  (A split whose events all sit, uncensored company only, at the largest time has
    no comparable pair either: the reference divides 0 by 0 there, this raises.)"""
    if comparable == 0:
        raise ValueError("Data has no comparable pairs, cannot estimate concordance index.")
    return (float(concordant) + 0.5 * float(tied_risk)) / float(comparable), concordant, discordant, tied_risk, tied_time


def concordance_index_censored(event, time, estimate, tied_tol=1e-8):
    """The reference's ``concordance_index_censored(event_indicator, event_time, estimate, tied_tol)`` on device tensors: the 5-tuple
    (cindex, concordant, discordant, tied_risk, tied_time).  ``estimate``: the risk (higher = earlier event): ``-y_pred`` serves the
    Cox evaluator's ``_c_index`` and the regression evaluator passes the negated predicted time the same way
    (eval/cindex.py:29-35, eval/evaluator_surv.py:329-332, 419-422)."""
    time, event, estimate = _as_tensor(time), _as_tensor(event), _as_tensor(estimate)
    _need_gpu(time, event, estimate)
    check = torch.stack([torch.isfinite(estimate.detach().reshape(-1).double()).all(), (event.detach().reshape(-1) != 0).any()])
    counts = concordance_counts(time, event, estimate, tied_tol)
    host = torch.cat([counts, check.to(torch.int64)]).cpu().tolist()          # the one copy
    if not host[5]:
        raise ValueError("Input contains NaN or infinity.")
    if estimate.numel() < 2:
        raise ValueError("Need a minimum of two samples")
    if not host[6]:
        raise ValueError("All samples are censored")
    return _cindex(*host[:5])


class SurvEvaluator:
    """``NLLSurv_Evaluator(prediction_type, backend != 'SurvivalEVAL')`` on the device.  ``compute`` takes the reference's ``data``
    dict with DEVICE tensors -- ``'y'`` [M, 2] = (t, e); ``'raw_y_hat'`` [M, K] logits (preferred: the converter is fused into the
    launch), else ``'y_hat'``; ``'avg_y_hat'`` replaces the prediction as in the reference; ``'uid'`` is ignored -- and returns the
    reference's keys as Python floats.  ``alpha`` / ``eps``: of ``loss_mle`` (the reference loads it with its defaults, 0 and 1e-7).

    Ext losses (``kws_ext_loss``: the handler's loss dict, the reference's objects or this package's -- attributes only): SurvIFMLE /
    SurvEMD on incidences come out of the rows launch; SurvMLE / SurvEMD on hazards and SurvT2I under either type out of the launches of
    ``vlsa_amd.losses`` (csrc/surv_objectives.hip), one ``.item()`` each; anything else is called as the reference calls it."""

    valid_metrics = ["c_index", "loss", "loss_mle", "loss_mle_org"]
    fused_ext_losses = ("SurvIFMLE", "SurvEMD")
    hazard_ext_losses = ("SurvMLE", "SurvEMD")          # under prediction_type = 'hazard': the per-sample launch of vlsa_amd.losses

    def __init__(self, prediction_type: str, backend: str = "none", alpha: float = 0.0, eps: float = 1e-7, tied_tol: float = 1e-8, **kws):
        assert prediction_type in ["hazard", "incidence"], "The `prediction_type` should be hazard or incidence."
        if backend == "SurvivalEVAL":
            raise NotImplementedError("the SurvivalEVAL metrics stay on the host: compute(..., ret_survival=True) returns the survival "
                                      "curves they start from")
        self.type, self.backend, self.kws = prediction_type, backend, kws
        self.alpha, self.eps, self.tied_tol = float(alpha), float(eps), float(tied_tol)

    def _check_metrics(self, metrics):
        for m in metrics:
            assert m in self.valid_metrics, f"[SurvEvaluator] got an invalid metric name: {m}."

    # ---- the launches ----
    _module_attrs = {"SurvMLE": ("alpha", "eps"), "SurvEMD": ("p", "raw_distance"), "SurvT2I": ("loss", "reduction")}

    def _by_module(self, name, func):
        """a loss OBJECT named SurvT2I, or SurvMLE / SurvEMD under 'hazard', carrying the attributes the launches read (a plain
        callable under one of these names is called as the reference calls it)"""
        if name != "SurvT2I" and not (self.type == "hazard" and name in self.hazard_ext_losses):
            return False
        return all(hasattr(func, a) for a in self._module_attrs[name])

    def _ext_spec(self, kws_ext_loss, kws):
        """(ext_mask, alpha, eps, p, raw_distance, w_ifmle, w_emd) of the ext losses the rows kernel evaluates, `modules` = the names
        the launches of vlsa_amd.losses evaluate (SurvMLE / SurvEMD on hazards, SurvT2I), and the names left to be called as the
        reference calls them"""
        spec = dict(mask=0, alpha=0.0, eps=1e-7, p=2, raw=1, w_ifmle=0.0, w_emd=0.0, modules=[])
        other = []
        for name, func in (kws_ext_loss or {}).items():
            if self._by_module(name, func):
                # evaluated by the launches of vlsa_amd.losses (surv_objectives.hip), whichever class the handler's object is
                if name != "SurvT2I" and getattr(func, "reduction", "mean") != "mean":
                    raise NotImplementedError(f"{name}: the evaluator covers reduction = 'mean', got {func.reduction!r}")
                if name == "SurvEMD" and func.p not in (1, 2):
                    raise NotImplementedError(f"SurvEMD: the kernel covers p = 1 and p = 2, got {func.p!r}")
                if name == "SurvT2I" and func.loss not in ("CL", "KL"):
                    raise NotImplementedError(f"Expected loss = CL or KL, but got {func.loss}.")
                spec["modules"].append(name)
                continue
            if name not in self.fused_ext_losses:
                other.append(name)
                continue
            if self.type != "incidence":
                raise NotImplementedError(f"{name} is evaluated for incidence predictions only")
            if getattr(func, "reduction", "mean") != "mean":
                raise NotImplementedError(f"{name}: the evaluator covers reduction = 'mean', got {func.reduction!r}")
            weight = float(kws["loss_weight"][name]) if "loss_weight" in kws else 1.0
            if name == "SurvIFMLE":
                spec.update(mask=spec["mask"] | 1, alpha=float(func.alpha), eps=float(func.eps), w_ifmle=weight)
            else:
                if func.p not in (1, 2):
                    raise NotImplementedError(f"SurvEMD: the kernel covers p = 1 and p = 2, got {func.p!r}")
                spec.update(mask=spec["mask"] | 2, p=int(func.p), raw=int(bool(func.raw_distance)), w_emd=weight)
        return spec, other

    def _launch(self, data, metrics, kws_ext_loss, ret_survival, kws):
        self._check_metrics(metrics)
        assert kws_ext_loss is None or isinstance(kws_ext_loss, dict)
        spec, other = self._ext_spec(kws_ext_loss, kws)
        y = _as_tensor(data["y"])
        if "avg_y_hat" in data:
            x, kind = data["avg_y_hat"], nat.EVAL_CONVERTED
        elif data.get("raw_y_hat") is not None:
            x, kind = data["raw_y_hat"], nat.EVAL_RAW
        else:
            x, kind = data["y_hat"], nat.EVAL_CONVERTED
        x = _as_tensor(x)
        _need_gpu(x, y)
        if x.dim() != 2 or y.dim() != 2 or y.shape[1] != 2:
            raise ValueError("expected predictions [M, K] and labels 'y' [M, 2] = (t, e)")
        lib = nat.load()
        x = x.detach().float().contiguous()
        M, K = x.shape
        if M < 1:
            raise ValueError("Need a minimum of two samples")
        t, e = _labels(y[:, 0].detach(), y[:, 1].detach(), M, x.device)
        ls, ls_value = kws.get("logit_scale", 10.0), 0.0
        if isinstance(ls, torch.Tensor):
            ls = ls.detach().to(device=x.device, dtype=torch.float32).reshape(-1)[:1].contiguous()
        else:
            ls, ls_value = None, float(ls)
        # one allocation: result words | est | time (all 8-byte), the curves apart
        buf = torch.empty(nat.EVAL_RESULT_WORDS + 2 * M, dtype=torch.float64, device=x.device)
        res, est, tm = buf[:nat.EVAL_RESULT_WORDS], buf[nat.EVAL_RESULT_WORDS:nat.EVAL_RESULT_WORDS + M], buf[nat.EVAL_RESULT_WORDS + M:]
        surv = torch.empty(M, K, dtype=torch.float32, device=x.device) if ret_survival else None
        nat.check(lib.vlsa_surv_eval_rows(_p(x), kind, _TYPES[self.type], _p(t), _p(e), M, K, self.alpha, self.eps, _p(ls), ls_value, 0,
                                          spec["mask"], spec["alpha"], spec["eps"], spec["p"], spec["raw"], spec["w_ifmle"], spec["w_emd"],
                                          _p(est), _p(tm), _p(surv), _p(res), _stream()), "vlsa_surv_eval_rows")
        if "c_index" in metrics:
            nat.check(lib.vlsa_concordance_pairs(_p(tm), _p(e), _p(est), M, self.tied_tol, _p(res[_COUNTERS]), 0, _stream()),
                      "vlsa_concordance_pairs")
        return res, est, surv, x, kind, t, e, other + spec["modules"]

    def _module_loss(self, name, func, data, x, kind, t, e, ls):
        """An ext loss of ``_ext_spec``'s `modules` as a 0-dim device tensor, unweighted: SurvMLE / SurvEMD on the hazards (the sigmoid
        fused in where x holds raw logits), SurvT2I on ``data['raw_y_hat']``"""
        from . import losses as L
        if name == "SurvT2I":
            raw = data.get("raw_y_hat")
            if raw is None:
                raise ValueError("SurvT2I is evaluated on data['raw_y_hat']")
            return L._launch_t2i(_as_tensor(raw), t, e, ls, False, func.loss, func.reduction, 1.0, want_grad=False)[0]
        conv = nat.CONV_SIGMOID if kind == nat.EVAL_RAW else nat.CONV_NONE
        if name == "SurvMLE":
            return L._launch_terms(x, t, e, conv, nat.SURV_MLE, None, func.alpha, func.eps, 2, True, 1.0, 0.0, want_grad=False)[0].mean()
        return L._launch_terms(x, t, e, conv, nat.SURV_MLE, ls, 0.0, 1e-7, func.p, func.raw_distance, 0.0, 1.0, want_grad=False)[1].mean()

    def compute_device(self, data, metrics, kws_ext_loss=None, **kws):
        """The launches of ``compute`` without the copy: the device result buffer, 16 float64 words laid out as ``vlsa_hip.h`` says
        (the pair counters are the int64 view of words 8 .. 12), for a loop that reads it later with ``read``.  Covers the metrics
        and the ext losses named SurvIFMLE / SurvEMD; any other ext loss needs ``compute``."""
        res, *_, other = self._launch(data, metrics, kws_ext_loss, False, kws)
        if other:
            raise NotImplementedError(f"compute_device evaluates {self.fused_ext_losses} only, got {other}")
        return res

    def read(self, result, metrics, kws_ext_loss=None):
        """The metrics dict from a result buffer of ``compute_device`` (one device-to-host copy where it is still on the device)."""
        host = result.cpu()
        sums = host.tolist()
        counts = host[_COUNTERS].view(torch.int64).tolist()
        M = int(sums[nat.EVAL_M])
        out = {}
        for m in metrics:
            if m == "c_index":
                # the reference's order of refusals: check_array, then eval/cindex.py:78-82, then 118-120
                if sums[nat.EVAL_NONFINITE] != 0:
                    raise ValueError("Input contains NaN or infinity.")
                if M < 2:
                    raise ValueError("Need a minimum of two samples")
                if sums[nat.EVAL_EVENTS] == 0:
                    raise ValueError("All samples are censored")
                out[m] = _cindex(*counts)[0]
            else:
                out[m] = sums[nat.EVAL_SUM_MLE if m == "loss_mle" else nat.EVAL_SUM_MLE_ORG] / M
        for name in (kws_ext_loss or {}):
            if name in self.fused_ext_losses:
                out["loss_" + name] = sums[nat.EVAL_SUM_IFMLE if name == "SurvIFMLE" else nat.EVAL_SUM_EMD] / M
        self.counts = dict(zip(("concordant", "discordant", "tied_risk", "tied_time", "comparable"), counts))
        return out

    def compute(self, data, metrics, kws_ext_loss=None, ret_survival=False, ret_risk=False, **kws):
        """``NLLSurv_Evaluator.compute``: {metric: float}, plus ``loss_<name>`` per entry of ``kws_ext_loss`` weighted by
        ``loss_weight[name]`` (``logit_scale``: the exponentiated scale, a float or a tensor, default 10).  ``ret_survival`` /
        ``ret_risk`` add the device tensors ``'survival_hat'`` [M, K] fp32 (clamped at 0, for SurvivalEVAL on the host) and
        ``'risk'`` [M] float64 (the estimate Harrell's C ranks by).  After the call ``self.counts`` holds the five pair counts."""
        res, est, surv, x, kind, t, e, other = self._launch(data, metrics, kws_ext_loss, ret_survival, kws)
        out = self.read(res, metrics, kws_ext_loss)
        if other:       # the reference's _eval_ext_loss (eval/evaluator_surv.py:198-212), on the device tensors
            weight = lambda name: kws["loss_weight"][name] if "loss_weight" in kws else 1  # noqa: E731
            ls = kws.get("logit_scale", 10.0)
            t1, e1 = t.unsqueeze(-1), e.unsqueeze(-1)
            y_hat = None
            for name in other:
                func = kws_ext_loss[name]
                if name == "QueryDiv":
                    loss = weight(name) * func()
                elif self._by_module(name, func):
                    loss = weight(name) * self._module_loss(name, func, data, x, kind, t, e, ls)
                elif name == "SurvT2I":
                    loss = weight(name) * func(data.get("raw_y_hat"), t1, e1, ls)
                else:
                    if y_hat is None:
                        y_hat = x if kind == nat.EVAL_CONVERTED else (torch.softmax(x, dim=-1) if self.type == "incidence" else torch.sigmoid(x))
                    loss = weight(name) * func(y_hat, t1, e1)
                out["loss_" + name] = loss.item()
            out = {k: out[k] for k in list(metrics) + ["loss_" + n for n in kws_ext_loss]}      # the reference's key order
        if ret_survival:
            out["survival_hat"] = surv
        if ret_risk:
            out["risk"] = est
        return out


# ---- the continuous heads: CoxSurv_Evaluator and RegSurv_Evaluator (eval/evaluator_surv.py:238-466) on a one-column prediction ----
def _column(data, M=None):
    """(y_hat [M] fp32, t [M] float64, e [M] fp32) of the reference's ``data`` dict: 'avg_y_hat' replaces 'y_hat' as in the reference"""
    y = _as_tensor(data["y"])
    x = _as_tensor(data["avg_y_hat"] if "avg_y_hat" in data else data["y_hat"])
    _need_gpu(x, y)
    if y.dim() != 2 or y.shape[1] != 2 or x.dim() not in (1, 2) or (x.dim() == 2 and x.shape[1] != 1):
        raise ValueError("expected a one-column prediction [M] or [M, 1] and labels 'y' [M, 2] = (t, e)")
    x = x.detach().reshape(-1).float().contiguous()
    M = x.numel()
    if M < 1:
        raise ValueError("Need a minimum of two samples")
    t = y[:, 0].detach().to(device=x.device, dtype=torch.float64).contiguous()
    e = y[:, 1].detach().to(device=x.device, dtype=torch.float32).contiguous()
    if t.numel() != M:
        raise ValueError("t and e must hold one entry per sample")
    return x, t, e


def _check_cindex(nonfinite, M, events):
    """the reference's order of refusals: check_array, then eval/cindex.py:78-82, then 118-120 (no comparable pair: ``_cindex``)"""
    if nonfinite != 0:
        raise ValueError("Input contains NaN or infinity.")
    if M < 2:
        raise ValueError("Need a minimum of two samples")
    if events == 0:
        raise ValueError("All samples are censored")


def cox_risk_sets(theta, t, e, cap=10.0):
    """D [M] float64 = sum_{j: t_j >= t_i} exp(min(theta_j, cap)) (``vlsa_cox_risk_sets``); theta fp32, t float64, e fp32, contiguous"""
    lib = nat.load()
    D = torch.empty(theta.numel(), dtype=torch.float64, device=theta.device)
    nat.check(lib.vlsa_cox_risk_sets(_p(theta), _p(t), _p(e), theta.numel(), float(cap), _p(D), _stream()), "vlsa_cox_risk_sets")
    return D


def cox_cum_hazard(t, e, D, query):
    """H [Q] float64 = sum_{i: e_i = 1, t_i <= query_q} 1 / D_i (``vlsa_cox_cum_hazard``)"""
    lib = nat.load()
    query = query.to(dtype=torch.float64).contiguous()
    H = torch.empty(query.numel(), dtype=torch.float64, device=t.device)
    nat.check(lib.vlsa_cox_cum_hazard(_p(t), _p(e), _p(D), t.numel(), _p(query), query.numel(), _p(H), _stream()), "vlsa_cox_cum_hazard")
    return H


class CoxSurvEvaluator:
    """``CoxSurv_Evaluator(backend != 'SurvivalEVAL')`` (eval/evaluator_surv.py:238-378) on the device: ``compute`` takes the reference's
    ``data`` dict with DEVICE tensors -- ``'y'`` [M, 2] = (t, e), ``'y_hat'`` or ``'avg_y_hat'`` [M, 1] or [M], ``'name'``; ``'uid'`` is
    ignored (the labels come from ``'y'``, not from a meta-data table) -- and returns ``c_index``, ``loss`` and ``loss_ple`` as Python
    floats.  Three launches -- the risk-set sums, the finishing sums, the pair counts -- and ONE copy of a 128-byte result buffer.

    ``c_index`` mirrors the reference's ``_c_index``: Harrell's C of the estimate ``-y_hat`` (eval/cindex.py:29-35).  ``SurvPLE`` drives
    y_hat UP for early events, so a head it trained scores 1 - C under this key; ``concordance_index_censored(e, t, y_hat)`` gives the
    other sign.  The Breslow baseline (eval/utils_coxph.py:193-236, theta uncapped) is fitted by ``fit_baseline`` -- which ``compute``
    runs itself when ``data['name'] == 'train'``, as the reference does -- with one ``torch.unique``, so one synchronisation per fit;
    ``compute(..., ret_survival=True)`` then adds ``'time_points'`` [U] and ``'survival_hat'`` [M, U] = exp(-H_u exp(y_hat_m)), float64,
    the curves ``_pre_compute`` hands SurvivalEVAL, and raises ``RuntimeError`` before a fit."""

    valid_metrics = ["c_index", "loss", "loss_ple"]
    CAP = 10.0                                # SurvPLE's CONSTANT

    def __init__(self, backend: str = "none", tied_tol: float = 1e-8, **kws):
        if backend == "SurvivalEVAL":
            raise NotImplementedError("the SurvivalEVAL metrics stay on the host: compute(..., ret_survival=True) returns the survival "
                                      "curves they start from")
        self.backend, self.kws, self.tied_tol = backend, kws, float(tied_tol)
        self.time_points = self.cum_hazard = None

    def _check_metrics(self, metrics):
        for m in metrics:
            assert m in self.valid_metrics, f"[CoxSurvEvaluator] got an invalid metric name: {m}."

    def fit_baseline(self, y_hat, t, e):
        """Breslow's estimator on a training split: stores its sorted unique times [U] and the cumulative baseline hazard there [U]"""
        y = torch.stack([_as_tensor(t).reshape(-1).double(), _as_tensor(e).reshape(-1).double()], dim=1)
        return self._fit(*_column({"y_hat": y_hat, "y": y}))

    def _fit(self, x, t, e):
        """``fit_baseline`` on converted tensors (``_column``)"""
        D = cox_risk_sets(x, t, e, float("inf"))
        self.time_points = torch.unique(t)        # sorted; the one synchronisation of a fit
        self.cum_hazard = cox_cum_hazard(t, e, D, self.time_points)
        return self

    def survival(self, y_hat):
        """[M, U] float64 curves S(u | x_m) = S_0(u) ^ exp(y_hat_m) at ``self.time_points``"""
        if self.cum_hazard is None:
            raise RuntimeError("CoxSurvEvaluator: no baseline yet -- call fit_baseline, or compute on data whose 'name' is 'train'")
        return torch.exp(-self.cum_hazard.view(1, -1) * torch.exp(_as_tensor(y_hat).detach().reshape(-1, 1).double()))

    def _launch(self, x, t, e, metrics):
        """the launches on converted tensors (``_column``): the device result buffer"""
        lib = nat.load()
        M = x.numel()
        res = torch.empty(nat.CEVAL_RESULT_WORDS, dtype=torch.float64, device=x.device)
        D = cox_risk_sets(x, t, e, self.CAP)
        nat.check(lib.vlsa_cox_finish(_p(x), _p(e), _p(D), M, self.CAP, _p(res), _stream()), "vlsa_cox_finish")
        if "c_index" in metrics:
            est = (-x).double()
            nat.check(lib.vlsa_concordance_pairs(_p(t), _p(e), _p(est), M, self.tied_tol, _p(res[nat.CEVAL_CONCORDANT:]), 0, _stream()),
                      "vlsa_concordance_pairs")
        return res

    def compute_device(self, data, metrics, **kws):
        """The launches of ``compute`` without the copy (and without a baseline fit): the device result buffer, laid out as
        ``vlsa_hip.h`` says (``VLSA_CEVAL_*``), for a loop that reads it later with ``read``."""
        self._check_metrics(metrics)
        return self._launch(*_column(data), metrics)

    def read(self, result, metrics):
        host = result.cpu()
        sums = host.tolist()
        counts = host[nat.CEVAL_CONCORDANT:nat.CEVAL_COMPARABLE + 1].view(torch.int64).tolist()
        M = int(sums[nat.CEVAL_M])
        out = {}
        for m in metrics:
            if m == "c_index":
                _check_cindex(sums[nat.CEVAL_NONFINITE], M, sums[nat.CEVAL_EVENTS])
                out[m] = _cindex(*counts)[0]
            else:
                out[m] = 0.0 - sums[nat.CEVAL_SUM_PLE] / M
        self.counts = dict(zip(("concordant", "discordant", "tied_risk", "tied_time", "comparable"), counts))
        return out

    def compute(self, data, metrics, ret_survival=False, **kws):
        self._check_metrics(metrics)
        x, t, e = _column(data)                  # the one conversion of the labels; the fit and the launches share it
        if data.get("name") == "train":
            self._fit(x, t, e)
        out = self.read(self._launch(x, t, e, metrics), metrics)
        if ret_survival:
            out["survival_hat"] = self.survival(x)
            out["time_points"] = self.time_points
        return out


def _fp32_reciprocal(n):
    """1 / n as the reference's rank_loss forms it: its pair weights ``pair_mask.float() / pair_mask.float().sum()`` are fp32 whatever
    the prediction's dtype, so the mean it returns is the sum times the fp32 rounding of 1 / n (loss/loss_surv.py:50-60)"""
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32))


class RegSurvEvaluator:
    """``RegSurv_Evaluator(end_time=...)`` (eval/evaluator_surv.py:381-466) on the device: its nine metrics from ``vlsa_reg_eval`` (every
    pair for ``loss_rank``, one workgroup for the rest, float64) and ``vlsa_concordance_pairs``, ONE copy of a 144-byte result buffer.
    ``alpha`` / ``gamma`` / ``norm``: of ``loss_recon`` (the reference loads it with its defaults, where it equals ``loss_recon_org``);
    ``rank_gamma`` / ``rank_norm``: of ``loss_rank``, which is the exact pair sum times the fp32 rounding of 1 / pairs, as the reference's
    fp32 pair weights make it (within 6e-8 of the mean, relative; exact counts up to 2^24 pairs).  An empty event or non-event group
    gives NaN, as the reference's mean of nothing.

    ``c_index``: the reference's own ``_c_index`` cannot run -- it passes ``type_pred='survival_time'`` into ``concordance_index``, which
    asserts ``'hazard_ratio'`` for a one-column prediction (eval/cindex.py:29-31).  This returns what the call yields without the
    assertion: Harrell's C of the estimate ``-y_hat``."""

    valid_metrics = ["c_index", "loss", "loss_rank", "loss_recon", "loss_recon_org", "event_t_rae", "nonevent_t_rae", "event_t_nre",
                     "nonevent_t_nre"]

    def __init__(self, end_time=None, alpha=0.0, gamma=1.0, norm="l1", rank_gamma=1.0, rank_norm="l1", tied_tol=1e-8, **kws):
        if end_time is None:
            raise KeyError("end_time")             # the reference reads kws['end_time']
        from .losses import _NORM
        if rank_norm not in _NORM:
            raise NotImplementedError("Arg. `norm` expected l1/l2, but got {}".format(rank_norm))
        self.end_time, self.kws, self.tied_tol = float(end_time), kws, float(tied_tol)
        self._spec = (float(rank_gamma), _NORM[rank_norm], float(alpha), float(gamma), _NORM["l2" if norm == "l2" else "l1"], self.end_time)

    def _check_metrics(self, metrics):
        for m in metrics:
            assert m in self.valid_metrics

    def compute_device(self, data, metrics, **kws):
        """The launches of ``compute`` without the copy: the device result buffer (``VLSA_REVAL_*``) for ``read``."""
        self._check_metrics(metrics)
        x, t, e = _column(data)
        lib = nat.load()
        M = x.numel()
        buf = torch.empty(nat.REVAL_RESULT_WORDS + 2 * M, dtype=torch.float64, device=x.device)       # result words | per-sample partials
        res = buf[:nat.REVAL_RESULT_WORDS]
        nat.check(lib.vlsa_reg_eval(_p(x), _p(t), _p(e), M, *self._spec, _p(buf[nat.REVAL_RESULT_WORDS:]), None, _p(res), _stream()),
                  "vlsa_reg_eval")
        if "c_index" in metrics:
            est = (-x).double()
            nat.check(lib.vlsa_concordance_pairs(_p(t), _p(e), _p(est), M, self.tied_tol, _p(res[nat.REVAL_CONCORDANT:]), 0, _stream()),
                      "vlsa_concordance_pairs")
        return res

    def read(self, result, metrics):
        host = result.cpu()
        s = host.tolist()
        counts = host[nat.REVAL_CONCORDANT:nat.REVAL_COMPARABLE + 1].view(torch.int64).tolist()
        M = int(s[nat.REVAL_M])
        mean = lambda total, n: total / n if n else float("nan")  # noqa: E731
        values = {"loss": lambda: s[nat.REVAL_RECON_ORG] / M, "loss_recon_org": lambda: s[nat.REVAL_RECON_ORG] / M,
                  "loss_recon": lambda: s[nat.REVAL_RECON] / M,
                  "loss_rank": lambda: s[nat.REVAL_RANK_NUM] * _fp32_reciprocal(s[nat.REVAL_RANK_PAIRS]) if s[nat.REVAL_RANK_PAIRS] else 0.0,
                  "event_t_rae": lambda: mean(s[nat.REVAL_EVT_RAE], s[nat.REVAL_N_EVT]),
                  "nonevent_t_rae": lambda: mean(s[nat.REVAL_NOEVT_RAE], s[nat.REVAL_N_NOEVT]),
                  "event_t_nre": lambda: mean(s[nat.REVAL_EVT_NRE], s[nat.REVAL_N_EVT]),
                  "nonevent_t_nre": lambda: mean(s[nat.REVAL_NOEVT_NRE], s[nat.REVAL_N_NOEVT])}
        out = {}
        for m in metrics:
            if m == "c_index":
                _check_cindex(s[nat.REVAL_NONFINITE], M, s[nat.REVAL_EVENTS])
                out[m] = _cindex(*counts)[0]
            else:
                out[m] = values[m]()
        self.counts = dict(zip(("concordant", "discordant", "tied_risk", "tied_time", "comparable"), counts))
        self.rank_pairs = int(s[nat.REVAL_RANK_PAIRS])
        return out

    def compute(self, data, metrics, **kws):
        return self.read(self.compute_device(data, metrics), metrics)
