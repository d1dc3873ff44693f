"""Scoring a split on the device: the reference's ``NLLSurv_Evaluator`` (eval/evaluator_surv.py:45-235, a backend other than
SurvivalEVAL) and its vendored ``concordance_index_censored`` (eval/cindex.py:152-207) on the [M, K] logits and (t, e) labels that are
already in HBM after an evaluation pass.  Two launches -- ``vlsa_surv_eval_rows`` (per sample, float64: converter, survival curve,
risk, loss sums) and ``vlsa_concordance_pairs`` (every pair, integer counts) -- and ONE device-to-host copy of a 128-byte result
buffer; Harrell's C is formed on the host from the exact counts.  No CPU fallback: a CPU tensor raises ``VlsaNativeError``.

What stays on the host: the SurvivalEVAL metrics (C on the mean survival time, IBS, MAE, D-calibration), which go through splines and
Kaplan-Meier fits of the training set; ``compute(..., ret_survival=True)`` hands back the clamped survival curves for them.
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
