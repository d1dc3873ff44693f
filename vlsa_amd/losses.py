"""Loss tail of the training step on the device, from the launches of ``csrc/surv_objectives.hip``: the handler's
[B, K] losses (runner/vlsa_handler.py:33-41, loss/utils.py:52-76) with the reference's constructor arguments and call signatures --
``SurvIFMLE`` (loss/loss_surv.py:127-169) on incidences, ``SurvMLE`` (loss/loss_surv.py:89-124) on hazards, ``SurvEMD``
(loss/loss_surv_ext.py:58-109) on either, ``SurvT2I`` (loss/loss_surv_ext.py:126-195) on the raw logits -- plus ``SurvObjective`` = the
handler's ``calc_objective_loss`` (runner/vlsa_handler.py:241-258) taking the RAW bag logits (softmax or sigmoid converter fused in).

Every module goes the same way: one preparation of the tensors (``_prep``, ``_scale``), a launch that returns the value AND its gradient
(``_launch_terms``: per-sample values and gradient rows, any batch; ``_launch_objective_terms``: the whole 'mean'-reduced objective in ONE
launch, up to ``ONE_LAUNCH_MAX_B`` samples), and one autograd function (``_LaunchFn``) that only scales the saved gradient by the
incoming one.

The continuous heads of runner/sa_handler.py -- ``SurvPLE`` (loss/loss_surv.py:172-209), ``rank_loss``, ``recon_loss`` and ``MSE_loss``
(lines 11-86) on a one-column prediction -- come from the launch of ``csrc/surv_pairs.hip``; ``SurvPairObjective`` is their
``calc_objective_loss``.
"""
from __future__ import annotations


import torch
import torch.nn as nn

from . import _native as nat
from .functional import _need_gpu, _p, _stream


_CONV = {"none": nat.CONV_NONE, "softmax": nat.CONV_SOFTMAX, "sigmoid": nat.CONV_SIGMOID}
_T2I_LOSS = {"CL": nat.T2I_CL, "KL": nat.T2I_KL}
ONE_LAUNCH_MAX_B = 4096         # vlsa_surv_objective_terms: one block walks the batch


def _prep(x, t, e):
    """(x fp32 [B, K], t int64 [B], e fp32 [B]) contiguous on x's device"""
    _need_gpu(x)
    x = x.detach().float().contiguous()
    if x.dim() != 2:
        raise ValueError("expected predictions [B, K]")
    B = x.shape[0]
    t = t.reshape(-1).to(device=x.device, dtype=torch.int64).contiguous()
    e = e.reshape(-1).to(device=x.device, dtype=torch.float32).contiguous()
    if t.numel() != B or e.numel() != B:
        raise ValueError("t and e must hold one entry per sample")
    return x, t, e


def _scale(ls, device):
    if ls is None:
        return None
    if not isinstance(ls, torch.Tensor):
        ls = torch.tensor(float(ls), device=device)
    return ls.detach().to(device=device, dtype=torch.float32).reshape(1).contiguous()


def _t2i_reduction(reduction):
    return nat.T2I_MEAN if reduction == "mean" else nat.T2I_SUM      # the reference sums under anything but 'mean'


def _launch_terms(x, t, e, conv, family, ls, alpha, eps, p, raw, w_main, w_emd, want_grad):
    """``vlsa_surv_terms``: per-sample likelihood term [B] (or None), per-sample SurvEMD [B] (or None), gradient rows [B, K]"""
    x, t, e = _prep(x, t, e)
    lib = nat.load()
    B, K = x.shape
    ls = _scale(ls, x.device)
    o1 = torch.empty(B, dtype=torch.float32, device=x.device) if w_main != 0 or w_emd == 0 else None     # (both weights zero: zeros)
    o2 = torch.empty(B, dtype=torch.float32, device=x.device) if w_emd != 0 else None
    g = torch.empty(B, K, dtype=torch.float32, device=x.device) if want_grad else None
    nat.check(lib.vlsa_surv_terms(_p(x), _p(t), _p(e), B, K, conv, family, _p(ls), float(alpha), float(eps), int(p), int(raw), float(w_main),
                                  float(w_emd), _p(o1), _p(o2), _p(g), _stream()), "vlsa_surv_terms")
    return o1, o2, g


def _launch_t2i(x, t, e, ls, ls_is_log, loss, reduction, weight, want_grad=True):
    """``vlsa_surv_t2i``: (weight * T2I as a 0-dim tensor, weight * d T2I / d x [B, K] or None) in two launches"""
    x, t, e = _prep(x, t, e)
    lib = nat.load()
    B, K = x.shape
    ls = _scale(ls, x.device)
    work = torch.empty(K * nat.T2I_WORK_PER_BIN, dtype=torch.float64, device=x.device)
    out = torch.empty(1 + (B * K if want_grad else 0), dtype=torch.float32, device=x.device)
    g = out[1:].view(B, K) if want_grad else None
    nat.check(lib.vlsa_surv_t2i(_p(x), _p(t), _p(e), B, K, _p(ls), int(ls_is_log), _T2I_LOSS[loss], _t2i_reduction(reduction), float(weight),
                                _p(work), _p(out), _p(g), _stream()), "vlsa_surv_t2i")
    return out[0], g


def _launch_objective_terms(x, t, e, ls, ls_is_log, spec):
    """``vlsa_surv_objective_terms``: (objective as a 0-dim tensor, d objective / d x [B, K]) in ONE launch; spec: SurvObjective._spec()"""
    x, t, e = _prep(x, t, e)
    lib = nat.load()
    B, K = x.shape
    ls = _scale(ls, x.device)
    out = torch.empty(1 + B * K, dtype=torch.float32, device=x.device)      # objective | gradient: one allocation
    g = out[1:].view(B, K)
    conv, family, alpha, eps, p, raw, w_main, w_emd, w_t2i, t2i_loss, t2i_reduction = spec
    nat.check(lib.vlsa_surv_objective_terms(_p(x), _p(t), _p(e), B, K, conv, family, _p(ls), int(ls_is_log), float(alpha), float(eps), int(p),
                                            int(raw), float(w_main), float(w_emd), float(w_t2i), _T2I_LOSS[t2i_loss],
                                            _t2i_reduction(t2i_reduction), _p(out), _p(g), _stream()), "vlsa_surv_objective_terms")
    return out[0], g


def _terms_rows(x, t, e, ls, conv, family, alpha, eps, p, raw, w_main, w_emd):
    """(per-sample loss [B] = w_main * main_i + w_emd * emd_i of either family, its gradient rows [B, K])"""
    o1, o2, g = _launch_terms(x, t, e, conv, family, ls, alpha, eps, p, raw, w_main, w_emd, want_grad=True)
    return (w_emd * o2 if o1 is None else w_main * o1 if o2 is None else w_main * o1 + w_emd * o2), g


class _LaunchFn(torch.autograd.Function):
    """``launch(x)`` -> (value: a scalar or one entry per sample, d value / d x [B, K]): the launches forward, one multiplication backward;
    differentiable w.r.t. the predictions only."""

    @staticmethod
    def forward(ctx, x, launch):
        value, g = launch(x)
        ctx.save_for_backward(g)
        return value

    @staticmethod
    def backward(ctx, dl):
        (g,) = ctx.saved_tensors
        return dl.reshape(-1, 1) * g, None


def _reduce(loss, reduction):
    if reduction == "mean":
        return loss.mean()
    if reduction == "sum":
        return loss.sum()
    return loss.reshape(-1, 1)  # the reference's 'none' keeps the [B, 1] column


class SurvIFMLE(nn.Module):
    def __init__(self, alpha=0.0, eps=1e-7, reduction="mean", **kws):
        super().__init__()
        assert reduction in ["sum", "mean", "none"]
        self.alpha, self.eps, self.reduction = alpha, eps, reduction

    def forward(self, incidence_hat, t, e, cur_alpha=None):
        alpha = self.alpha if cur_alpha is None else cur_alpha
        loss = _LaunchFn.apply(incidence_hat, lambda x: _terms_rows(x, t, e, None, nat.CONV_NONE, nat.SURV_IFMLE, alpha, self.eps, 2, True, 1.0, 0.0))
        return _reduce(loss, self.reduction)


class SurvEMD(nn.Module):
    def __init__(self, p=2, raw_distance=True, reduction="mean", **kws):
        super().__init__()
        assert reduction in ["mean", "sum", "none"]
        if p not in (1, 2):
            raise NotImplementedError("the fused kernel covers p = 1 and p = 2 (cfg_vlsa_conch.yaml uses 2)")
        self.p, self.raw_distance, self.reduction = p, raw_distance, reduction

    def forward(self, y_hat, t, e, cur_logit_scale=10.0):
        loss = _LaunchFn.apply(y_hat, lambda x: _terms_rows(x, t, e, cur_logit_scale, nat.CONV_NONE, nat.SURV_IFMLE, 0.0, 1e-7, self.p,
                                                           self.raw_distance, 0.0, 1.0))
        if self.reduction == "mean":
            return loss.mean()
        if self.reduction == "sum":
            return loss.sum()
        return loss


class SurvMLE(nn.Module):
    """The reference's ``SurvMLE`` (loss/loss_surv.py:89-124) on hazards [B, K] (converted by the sigmoid): the mean over the batch."""

    def __init__(self, alpha=0.0, eps=1e-7, **kws):
        super().__init__()
        self.alpha, self.eps = alpha, eps

    def forward(self, hazards_hat, t, e, cur_alpha=None):
        alpha = self.alpha if cur_alpha is None else cur_alpha
        return _LaunchFn.apply(hazards_hat, lambda x: _terms_rows(x, t, e, None, nat.CONV_NONE, nat.SURV_MLE, alpha, self.eps, 2, True, 1.0, 0.0)).mean()


class SurvT2I(nn.Module):
    """The reference's ``SurvT2I`` (loss/loss_surv_ext.py:126-195) on the RAW logits [B, K], without its loop over the bins and without
    a host synchronisation.  One difference: a batch without a counted bin (no event) gives a zero TENSOR whose gradient is zero,
    where the reference returns the Python float ``0.0``."""

    def __init__(self, loss="CL", reduction="mean", **kws):
        super().__init__()
        if loss not in _T2I_LOSS:
            raise NotImplementedError(f"Expected loss = CL or KL, but got {loss}.")
        self.loss, self.reduction = loss, reduction

    def forward(self, raw_y_hat, t, e, cur_logit_scale=10.0):
        return _LaunchFn.apply(raw_y_hat, lambda x: _launch_t2i(x, t, e, cur_logit_scale, False, self.loss, self.reduction, 1.0))


class SurvObjective(nn.Module):
    """weight_ifmle * SurvIFMLE(softmax(raw)) + weight_emd * SurvEMD(softmax(raw)), both 'mean'-reduced, from the raw
    [B, K] logits in one launch (``label``: [B, 2] = (t, e) as in the handler, or t and e separately).

    The keyword-only arguments select the handler's other objectives (``calc_objective_loss``, runner/vlsa_handler.py:241-258):
    ``converter='sigmoid'`` with ``weight_mle`` is the hazard family, weight_mle * SurvMLE(sigmoid(raw)) + weight_emd *
    SurvEMD(sigmoid(raw)); ``weight_t2i`` adds weight_t2i * SurvT2I(raw) in its ``t2i_loss`` ('CL' / 'KL') and ``t2i_reduction``
    ('mean' / 'sum') form.  Every objective is one launch (``vlsa_surv_objective_terms``) up to 4096 samples; above, the per-sample
    launch, the two of SurvT2I and torch adds."""

    def __init__(self, weight_ifmle=1.0, weight_emd=1.0, alpha=0.0, eps=1e-7, p=2, raw_distance=True, *, converter="softmax",
                 weight_mle=0.0, weight_t2i=0.0, t2i_loss="CL", t2i_reduction="mean"):
        super().__init__()
        if p not in (1, 2):
            raise NotImplementedError("the fused kernel covers p = 1 and p = 2")
        self.w1, self.w2, self.alpha, self.eps, self.p, self.raw = weight_ifmle, weight_emd, alpha, eps, p, raw_distance
        if converter not in ("softmax", "sigmoid"):
            raise ValueError(f"converter: 'softmax' or 'sigmoid' (the objective takes raw logits), got {converter!r}")
        if converter == "sigmoid" and weight_ifmle != 0:
            raise ValueError("SurvIFMLE needs net_output_converter = softmax (the handler's _check_arguments): pass weight_ifmle=0 with "
                             "converter='sigmoid'")
        if converter == "softmax" and weight_mle != 0:
            raise ValueError("SurvMLE needs net_output_converter = sigmoid (the handler's _check_arguments): pass converter='sigmoid'")
        if t2i_loss not in _T2I_LOSS:
            raise NotImplementedError(f"Expected loss = CL or KL, but got {t2i_loss}.")
        self.converter, self.w_mle, self.w_t2i, self.t2i_loss, self.t2i_reduction = converter, weight_mle, weight_t2i, t2i_loss, t2i_reduction

    @classmethod
    def from_handler(cls, loss, loss_weight, converter):
        """The objective of a handler's ``self.loss`` (name -> loss object, the reference's classes or this module's), its
        ``self.loss_weight`` and ``net_output_converter``.  Refuses with ``NotImplementedError`` what the launches do not cover."""
        kws = dict(weight_ifmle=0.0, weight_emd=0.0, converter=converter)
        for name, func in loss.items():
            weight = float(loss_weight[name])
            if name in ("SurvIFMLE", "SurvMLE", "SurvEMD") and getattr(func, "reduction", "mean") != "mean":
                raise NotImplementedError(f"{name}: the launches cover reduction = 'mean', got {func.reduction!r}")
            if name in ("SurvIFMLE", "SurvMLE"):
                kws.update(alpha=float(func.alpha), eps=float(func.eps))
                kws["weight_ifmle" if name == "SurvIFMLE" else "weight_mle"] = weight
            elif name == "SurvEMD":
                if func.p not in (1, 2):
                    raise NotImplementedError(f"SurvEMD: the launches cover p = 1 and p = 2, got {func.p!r}")
                kws.update(weight_emd=weight, p=int(func.p), raw_distance=bool(func.raw_distance))
            elif name == "SurvT2I":
                kws.update(weight_t2i=weight, t2i_loss=func.loss, t2i_reduction=func.reduction)
            else:
                raise NotImplementedError(f"{name} is not part of the launch (QueryDiv depends on the queries, not on the logits: add it apart)")
        return cls(**kws)

    def _spec(self):
        hazard = self.converter == "sigmoid"
        return (_CONV[self.converter], nat.SURV_MLE if hazard else nat.SURV_IFMLE, self.alpha, self.eps, self.p, self.raw,
                self.w_mle if hazard else self.w1, self.w2, self.w_t2i, self.t2i_loss, self.t2i_reduction)

    def forward(self, raw_pred, t, e=None, cur_logit_scale=10.0, log_logit_scale=None):
        """cur_logit_scale: exp(logit_scale) as the handler passes it (``net.get_logit_scale()``); log_logit_scale: the raw parameter
        instead (exponentiated inside the launch: one kernel less per step; no gradient flows into it either way -- the reference detaches it)."""
        if e is None:
            t, e = t[:, 0], t[:, 1]
        ls, is_log = (log_logit_scale, True) if log_logit_scale is not None else (cur_logit_scale, False)
        if isinstance(ls, torch.Tensor) and raw_pred.is_cuda and raw_pred.dim() == 2 and raw_pred.shape[0] <= ONE_LAUNCH_MAX_B:
            return _LaunchFn.apply(raw_pred, lambda x: _launch_objective_terms(x, t, e, ls, is_log, self._spec()))
        if is_log:
            ls = ls.detach().exp() if isinstance(ls, torch.Tensor) else float(torch.tensor(ls).exp())
        conv, family, alpha, eps, p, raw, w_main, w_emd, w_t2i, t2i_loss, t2i_reduction = self._spec()
        loss = _LaunchFn.apply(raw_pred, lambda x: _terms_rows(x, t, e, ls, conv, family, alpha, eps, p, raw, w_main, w_emd)).mean()
        if w_t2i != 0:
            loss = loss + _LaunchFn.apply(raw_pred, lambda x: _launch_t2i(x, t, e, ls, False, t2i_loss, t2i_reduction, w_t2i))
        return loss

    def value_and_grad(self, raw_pred, t, e=None, log_logit_scale=None):
        """(objective, d objective / d raw_pred) from the one launch, outside autograd -- for a caller that owns the step and starts the
        backward pass itself with ``raw_pred.backward(grad)`` (``vlsa_amd.train_step.TrainStep``): ``loss.backward()`` costs two more
        launches (the ones_like seed and its product with the saved gradient), ~10 us of a graph-replayed step.  [B, K] logits on the
        GPU, the raw (log) logit scale as a tensor."""
        if e is None:
            t, e = t[:, 0], t[:, 1]
        # Above ONE_LAUNCH_MAX_B samples the objectives differ, and callers rely on both: SurvIFMLE + SurvEMD without SurvT2I -- the objective
        # this method was written for -- has only the one launch, which refuses such a batch (VlsaNativeError); the hazard family and
        # anything with SurvT2I fall back to the launches of the autograd route.
        if raw_pred.shape[0] <= ONE_LAUNCH_MAX_B or (self.converter == "softmax" and self.w_t2i == 0):
            return _launch_objective_terms(raw_pred, t, e, log_logit_scale, True, self._spec())
        conv, family, alpha, eps, p, raw, w_main, w_emd, w_t2i, t2i_loss, t2i_reduction = self._spec()
        rows, g = _terms_rows(raw_pred, t, e, log_logit_scale.detach().exp(), conv, family, alpha, eps, p, raw, w_main, w_emd)
        value, g = rows.mean(), g / g.shape[0]
        if w_t2i != 0:
            v2, g2 = _launch_t2i(raw_pred, t, e, log_logit_scale, True, t2i_loss, t2i_reduction, w_t2i)
            value, g = value + v2, g + g2
        return value, g


# ---- the continuous heads (runner/sa_handler.py: loss_type SurvPLE, or recon_loss / rank_loss / MSE_loss, on a one-column prediction
# with net_output_converter None): csrc/surv_pairs.hip, value + every term's value + gradient in ONE launch up to 4096 samples,
# the split launches above ----
_NORM = {"l1": nat.PAIR_NORM_L1, "l2": nat.PAIR_NORM_L2}
PAIR_TERMS = {"SurvPLE": nat.PAIR_OBJ_PLE, "rank_loss": nat.PAIR_OBJ_RANK, "recon_loss": nat.PAIR_OBJ_RECON, "MSE_loss": nat.PAIR_OBJ_MSE}


def _pair_spec(w_ple=0.0, w_rank=0.0, w_recon=0.0, w_mse=0.0, rank_gamma=1.0, rank_norm="l1", recon_alpha=0.0, recon_gamma=1.0,
               recon_norm="l1", mse_include_censored=False):
    """the launch's arguments behind the tensors; recon_loss squares under 'l2' and takes anything else as l1, as the reference does"""
    if rank_norm not in _NORM:
        raise NotImplementedError("Arg. `norm` expected l1/l2, but got {}".format(rank_norm))
    return (float(w_ple), float(w_rank), float(w_recon), float(w_mse), float(rank_gamma), _NORM[rank_norm], float(recon_alpha),
            float(recon_gamma), _NORM["l2" if recon_norm == "l2" else "l1"], int(bool(mse_include_censored)))


def _launch_pair(pred, t, e, spec, want_grad=True):
    """``vlsa_surv_pair_objective``: (the launch's fp32 result words [PAIR_OBJ_WORDS] -- the objective, the four terms, the number of
    rank pairs --, d objective / d pred in pred's shape or None).  pred: [B] or [B, 1]; t: fp32 or fp64 stay as they are, any other
    dtype is compared as fp64; e: 0 / 1."""
    _need_gpu(pred)
    if pred.dim() not in (1, 2) or (pred.dim() == 2 and pred.shape[1] != 1):
        raise ValueError("expected a one-column prediction, [B] or [B, 1]")
    lib = nat.load()
    x = pred.detach().float().contiguous()
    B = x.numel()
    t = t.detach().reshape(-1).to(device=x.device)
    t = (t if t.dtype in (torch.float32, torch.float64) else t.double()).contiguous()
    e = e.detach().reshape(-1).to(device=x.device, dtype=torch.float32).contiguous()
    if t.numel() != B or e.numel() != B:
        raise ValueError("t and e must hold one entry per sample")
    out = torch.empty(nat.PAIR_OBJ_WORDS + (B if want_grad else 0), dtype=torch.float32, device=x.device)     # words | gradient: one allocation
    g = out[nat.PAIR_OBJ_WORDS:] if want_grad else None
    nat.check(lib.vlsa_surv_pair_objective(_p(x), _p(t), nat.PAIR_TIME_F64 if t.dtype == torch.float64 else nat.PAIR_TIME_F32, _p(e), B, *spec,
                                           _p(out), _p(g), _stream()), "vlsa_surv_pair_objective")
    return out[:nat.PAIR_OBJ_WORDS], (g.view(pred.shape) if want_grad else None)


def _launch_pair_split(pred, t, e, spec, want_grad=True):
    """``_launch_pair`` for a batch above ``PAIR_MAX_B`` samples: the split launches of csrc/surv_pairs.hip -- the risk-set sums and the
    cumulative hazard at the samples' own times (SurvPLE), every rank pair with the per-sample gradient (``vlsa_reg_eval``) -- in
    float64, joined by element-wise torch ops on [B] vectors (recon_loss and MSE_loss are element-wise altogether).  No
    synchronisation; the result words are fp32 as the one launch writes them."""
    from .evaluate import cox_cum_hazard, cox_risk_sets
    _need_gpu(pred)
    if pred.dim() not in (1, 2) or (pred.dim() == 2 and pred.shape[1] != 1):
        raise ValueError("expected a one-column prediction, [B] or [B, 1]")
    lib = nat.load()
    x = pred.detach().reshape(-1).float().contiguous()
    B = x.numel()
    t = t.detach().reshape(-1).to(device=x.device, dtype=torch.float64).contiguous()
    e = e.detach().reshape(-1).to(device=x.device, dtype=torch.float32).contiguous()
    if t.numel() != B or e.numel() != B:
        raise ValueError("t and e must hold one entry per sample")
    w_ple, w_rank, w_recon, w_mse, rank_gamma, rank_norm, recon_alpha, recon_gamma, recon_norm, mse_censored = spec
    p, ed = x.double(), e.double()
    words = torch.zeros(nat.PAIR_OBJ_WORDS, dtype=torch.float64, device=x.device)
    g = torch.zeros(B, dtype=torch.float64, device=x.device)
    if w_ple != 0:
        D = cox_risk_sets(x, t, e, 10.0)
        res = torch.empty(nat.CEVAL_RESULT_WORDS, dtype=torch.float64, device=x.device)
        nat.check(lib.vlsa_cox_finish(_p(x), _p(e), _p(D), B, 10.0, _p(res), _stream()), "vlsa_cox_finish")
        words[nat.PAIR_OBJ_PLE] = 0.0 - res[nat.CEVAL_SUM_PLE] / B
        if want_grad:
            H = cox_cum_hazard(t, e, D, t)
            g += w_ple * torch.where(x > 10.0, torch.zeros_like(p), -(ed - torch.exp(p.clamp(max=10.0)) * H) / B)
    if w_rank != 0:
        buf = torch.empty(nat.REVAL_RESULT_WORDS + 3 * B, dtype=torch.float64, device=x.device)     # result words | partials | gradient
        res, rg = buf[:nat.REVAL_RESULT_WORDS], buf[nat.REVAL_RESULT_WORDS + 2 * B:]
        nat.check(lib.vlsa_reg_eval(_p(x), _p(t), _p(e), B, rank_gamma, rank_norm, recon_alpha, recon_gamma, recon_norm, 1.0,
                                    _p(buf[nat.REVAL_RESULT_WORDS:]), _p(rg), _p(res), _stream()), "vlsa_reg_eval")
        pairs = res[nat.REVAL_RANK_PAIRS]
        words[nat.PAIR_OBJ_RANK] = res[nat.REVAL_RANK_NUM] / pairs.clamp(min=1.0)       # no pair: the numerator is 0 too
        words[nat.PAIR_OBJ_PAIRS] = pairs
        g += w_rank * rg / pairs.clamp(min=1.0)
    d = p - t
    if w_recon != 0:
        l2 = recon_norm == nat.PAIR_NORM_L2
        x_c = recon_gamma - d
        obs, cen = ed * d.abs(), (1.0 - ed) * x_c.clamp(min=0.0)
        d_obs, d_cen = ed * torch.sign(d), -(1.0 - ed) * (x_c > 0)
        if l2:
            d_obs, d_cen, obs, cen = 2.0 * obs * d_obs, 2.0 * cen * d_cen, obs * obs, cen * cen
        words[nat.PAIR_OBJ_RECON] = ((1.0 - recon_alpha) * (obs + cen) + recon_alpha * obs).sum() / B
        g += w_recon * ((1.0 - recon_alpha) * (d_obs + d_cen) + recon_alpha * d_obs) / B
    if w_mse != 0:
        w = ed + (1.0 - ed if mse_censored else 0.0)
        words[nat.PAIR_OBJ_MSE] = (w * d * d).sum() / B
        g += w_mse * 2.0 * w * d / B
    words[nat.PAIR_OBJ_TOTAL] = (w_ple * words[nat.PAIR_OBJ_PLE] + w_rank * words[nat.PAIR_OBJ_RANK] + w_recon * words[nat.PAIR_OBJ_RECON]
                                 + w_mse * words[nat.PAIR_OBJ_MSE])
    return words.float(), (g.float().view(pred.shape) if want_grad else None)


def _pair_route(pred):
    return _launch_pair if pred.numel() <= nat.PAIR_MAX_B else _launch_pair_split


class _PairFn(torch.autograd.Function):
    """one result word of the launch as a 0-dim tensor, differentiable w.r.t. the prediction only: the launch forward, one
    multiplication backward"""

    @staticmethod
    def forward(ctx, pred, t, e, spec, word):
        words, g = _pair_route(pred)(pred, t, e, spec)
        ctx.save_for_backward(g)
        return words[word]

    @staticmethod
    def backward(ctx, dl):
        (g,) = ctx.saved_tensors
        return dl * g, None, None, None, None


def recon_loss(pred_t, t, e, alpha=0.0, gamma=1.0, norm="l1", cur_alpha=None, **kws):
    """The reference's ``recon_loss`` (loss/loss_surv.py:11-31): mean_i (1 - alpha) (obs_i + cen_i) + alpha obs_i."""
    spec = _pair_spec(w_recon=1.0, recon_alpha=alpha if cur_alpha is None else cur_alpha, recon_gamma=gamma, recon_norm=norm)
    return _PairFn.apply(pred_t, t, e, spec, nat.PAIR_OBJ_RECON)


def rank_loss(pred_t, t, e, gamma=1, norm="l1", add_weight=False, **kws):
    """The reference's ``rank_loss`` (loss/loss_surv.py:33-70) without its three [B, B] matrices.  Two differences: a batch without a
    pair gives a 0-dim zero whose gradient is zero (the reference: ``Tensor([0.])`` outside the graph), and ``add_weight=True`` is
    refused -- its softmax weights carry a gradient of their own that the launch does not form."""
    if add_weight:
        raise NotImplementedError("rank_loss(add_weight=True) is not part of the launch")
    return _PairFn.apply(pred_t, t, e, _pair_spec(w_rank=1.0, rank_gamma=gamma, rank_norm=norm), nat.PAIR_OBJ_RANK)


def MSE_loss(pred_t, t, e, include_censored=False, **kws):
    """The reference's ``MSE_loss`` (loss/loss_surv.py:72-86)."""
    return _PairFn.apply(pred_t, t, e, _pair_spec(w_mse=1.0, mse_include_censored=include_censored), nat.PAIR_OBJ_MSE)


class SurvPLE(nn.Module):
    """The reference's ``SurvPLE`` (loss/loss_surv.py:172-209) without its B x B Python loop.  One difference: a batch without an event
    gives ``0.`` where the reference gives ``-0.``."""

    def __init__(self, **kws):
        super().__init__()
        self.CONSTANT = torch.tensor(10.0)      # the cap lives in the kernel; kept for a caller that reads it

    def forward(self, y_hat, T, E):
        return _PairFn.apply(y_hat, T, E, _pair_spec(w_ple=1.0), nat.PAIR_OBJ_PLE)


class SurvPairObjective(nn.Module):
    """``calc_objective_loss`` of the continuous heads (runner/sa_handler.py:172-180 with the identity converter): weight_ple * SurvPLE +
    weight_rank * rank_loss + weight_recon * recon_loss + weight_mse * MSE_loss of a [B] or [B, 1] prediction, value and gradient in ONE
    launch (``vlsa_surv_pair_objective``).  ``label``: [B, 2] = (t, e) as the handler passes it, or t and e separately.  Above 4096
    samples the split launches take over (``_launch_pair_split``: float64 pair sums, torch adds).  The differences from the reference are those of
    ``rank_loss`` and ``SurvPLE`` above.  After a call ``self.terms`` holds the launch's result words on the device (``PAIR_TERMS``
    names the index of each term's unweighted value): the terms come out of the same launch, without a copy."""

    def __init__(self, weight_ple=0.0, weight_rank=0.0, weight_recon=0.0, weight_mse=0.0, *, rank_gamma=1.0, rank_norm="l1",
                 rank_add_weight=False, recon_alpha=0.0, recon_gamma=1.0, recon_norm="l1", mse_include_censored=False):
        super().__init__()
        if rank_add_weight:
            raise NotImplementedError("rank_loss(add_weight=True) is not part of the launch")
        self.weights = dict(SurvPLE=float(weight_ple), rank_loss=float(weight_rank), recon_loss=float(weight_recon), MSE_loss=float(weight_mse))
        self.options = dict(rank_gamma=rank_gamma, rank_norm=rank_norm, recon_alpha=recon_alpha, recon_gamma=recon_gamma,
                            recon_norm=recon_norm, mse_include_censored=mse_include_censored)
        self._spec = _pair_spec(weight_ple, weight_rank, weight_recon, weight_mse, **self.options)
        self.terms = None

    _handler_options = {"SurvPLE": {}, "rank_loss": {"gamma": "rank_gamma", "norm": "rank_norm", "add_weight": "rank_add_weight"},
                        "recon_loss": {"alpha": "recon_alpha", "gamma": "recon_gamma", "norm": "recon_norm"},
                        "MSE_loss": {"include_censored": "mse_include_censored"}}
    _handler_weight = {"SurvPLE": "weight_ple", "rank_loss": "weight_rank", "recon_loss": "weight_recon", "MSE_loss": "weight_mse"}

    @classmethod
    def from_handler(cls, loss, loss_weight, converter):
        """The objective of a handler's ``self.loss`` (name -> ``functools.partial`` of a loss function, whose ``.keywords`` are read, or
        a SurvPLE object: the reference's or this module's), its ``self.loss_weight`` and ``net_output_converter``.  Refuses an unknown
        name and ``add_weight=True`` with ``NotImplementedError``, a converter other than ``None`` with ``ValueError`` (the handler's own
        check, runner/sa_handler.py:38-40)."""
        if converter is not None:
            raise ValueError(f"the continuous heads need net_output_converter = None (the handler's _check_arguments), got {converter!r}")
        kws = {}
        for name, func in loss.items():
            if name not in cls._handler_options:
                raise NotImplementedError(f"{name} is not part of the launch ({', '.join(cls._handler_options)})")
            given = getattr(func, "keywords", None) or {}
            kws.update({mine: given[theirs] for theirs, mine in cls._handler_options[name].items() if theirs in given})
            kws[cls._handler_weight[name]] = float(loss_weight[name])
        return cls(**kws)

    def forward(self, pred, t, e=None):
        if e is None:
            t, e = t[:, 0], t[:, 1]
        return _PairFn.apply(pred, t, e, self._spec, nat.PAIR_OBJ_TOTAL)

    def value_and_grad(self, pred, t, e=None):
        """(objective, d objective / d pred in pred's shape) from the one launch, outside autograd -- for a caller that starts the
        backward pass itself with ``pred.backward(grad)``."""
        if e is None:
            t, e = t[:, 0], t[:, 1]
        self.terms, g = _pair_route(pred)(pred, t, e, self._spec)
        return self.terms[nat.PAIR_OBJ_TOTAL], g
