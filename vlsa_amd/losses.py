"""Loss tail of the training step on the device: ``SurvIFMLE`` (loss/loss_surv.py:127-169) and ``SurvEMD``
(loss/loss_surv_ext.py:58-109) with the reference's constructor arguments and call signatures, plus ``SurvObjective`` =
the handler's ``calc_objective_loss`` for ``loss_type: SurvIFMLE-SurvEMD`` (runner/vlsa_handler.py:241-258) taking the RAW
bag logits (softmax converter fused in).  Forward value and gradient come from ONE kernel launch (``vlsa_surv_loss``);
autograd only scales the saved gradient by the incoming one.

The handler's other objectives (runner/vlsa_handler.py:33-41, loss/utils.py:52-76) come from the launches of
``csrc/surv_objectives.hip``: the hazard family -- ``SurvMLE`` (loss/loss_surv.py:89-124) behind the sigmoid converter, ``SurvEMD`` on
the hazards -- and ``SurvT2I`` (loss/loss_surv_ext.py:126-195).  ``SurvObjective(converter=..., weight_mle=..., weight_t2i=...)`` takes
them in one launch too; with its defaults it issues exactly the launch it always issued.
"""
from __future__ import annotations


import torch
import torch.nn as nn

from . import _native as nat
from .functional import _need_gpu, _p, _stream


def _launch(x, t, e, from_logits, ls, alpha, eps, p, raw, w_ifmle, w_emd, want_grad):
    _need_gpu(x)
    lib = nat.load()
    x = x.detach().float().contiguous()
    B, K = x.shape
    t = t.reshape(-1).to(device=x.device, dtype=torch.int64).contiguous()
    e = e.reshape(-1).to(device=x.device, dtype=torch.float32).contiguous()
    if t.numel() != B or e.numel() != B:
        raise ValueError("t and e must hold one entry per sample")
    if ls is not None and not isinstance(ls, torch.Tensor):
        ls = torch.tensor(float(ls), device=x.device)
    if ls is not None:
        ls = ls.detach().to(device=x.device, dtype=torch.float32).reshape(1).contiguous()
    o1 = torch.empty(B, dtype=torch.float32, device=x.device) if w_ifmle != 0 else None
    o2 = torch.empty(B, dtype=torch.float32, device=x.device) if w_emd != 0 else None
    g = torch.empty(B, K, dtype=torch.float32, device=x.device) if want_grad else None
    nat.check(lib.vlsa_surv_loss(_p(x), _p(t), _p(e), B, K, int(from_logits), _p(ls), float(alpha), float(eps), int(p),
                                 int(raw), float(w_ifmle), float(w_emd), _p(o1), _p(o2), _p(g), _stream()), "vlsa_surv_loss")
    return o1, o2, g


class _SurvLossFn(torch.autograd.Function):
    """per-sample loss [B] = w_ifmle * ifmle_i + w_emd * emd_i, differentiable w.r.t. the predictions only."""

    @staticmethod
    def forward(ctx, x, t, e, ls, from_logits, alpha, eps, p, raw, w_ifmle, w_emd):
        o1, o2, g = _launch(x, t, e, from_logits, ls, alpha, eps, p, raw, w_ifmle, w_emd, want_grad=True)
        ctx.save_for_backward(g)
        if o1 is None or o2 is None:
            return w_emd * o2 if o1 is None else w_ifmle * o1
        return w_ifmle * o1 + w_emd * o2

    @staticmethod
    def backward(ctx, dl):
        (g,) = ctx.saved_tensors
        return (dl.reshape(-1, 1) * g,) + (None,) * 10


class _SurvObjectiveFn(torch.autograd.Function):
    """mean_i (w_ifmle ifmle_i + w_emd emd_i) from the raw logits: ONE launch forward (``vlsa_surv_objective``: value, gradient and the
    mean over the batch; optionally the exp of the raw logit scale), one multiplication backward."""

    @staticmethod
    def forward(ctx, x, t, e, ls, ls_is_log, alpha, eps, p, raw, w_ifmle, w_emd):
        _need_gpu(x)
        lib = nat.load()
        x = x.detach().float().contiguous()
        B, K = x.shape
        t = t.reshape(-1).to(device=x.device, dtype=torch.int64).contiguous()
        e = e.reshape(-1).to(device=x.device, dtype=torch.float32).contiguous()
        if t.numel() != B or e.numel() != B:
            raise ValueError("t and e must hold one entry per sample")
        ls = ls.detach().to(device=x.device, dtype=torch.float32).reshape(1).contiguous()
        out = torch.empty(1 + B * K, dtype=torch.float32, device=x.device)      # objective | gradient: one allocation
        g = out[1:].view(B, K)
        nat.check(lib.vlsa_surv_objective(_p(x), _p(t), _p(e), B, K, 1, _p(ls), int(ls_is_log), float(alpha), float(eps), int(p), int(raw),
                                          float(w_ifmle), float(w_emd), _p(out), _p(g), _stream()), "vlsa_surv_objective")
        ctx.save_for_backward(g)
        return out[0]

    @staticmethod
    def backward(ctx, dl):
        (g,) = ctx.saved_tensors
        return (dl * g,) + (None,) * 10


_CONV = {"none": nat.CONV_NONE, "softmax": nat.CONV_SOFTMAX, "sigmoid": nat.CONV_SIGMOID}
_T2I_LOSS = {"CL": nat.T2I_CL, "KL": nat.T2I_KL}


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
        loss = _SurvLossFn.apply(incidence_hat, t, e, None, False, alpha, self.eps, 2, True, 1.0, 0.0)
        return _reduce(loss, self.reduction)


class SurvEMD(nn.Module):
    def __init__(self, p=2, raw_distance=True, reduction="mean", **kws):
        super().__init__()
        assert reduction in ["mean", "sum", "none"]
        if p not in (1, 2):
            raise NotImplementedError("the fused kernel covers p = 1 and p = 2 (cfg_vlsa_conch.yaml uses 2)")
        self.p, self.raw_distance, self.reduction = p, raw_distance, reduction

    def forward(self, y_hat, t, e, cur_logit_scale=10.0):
        loss = _SurvLossFn.apply(y_hat, t, e, cur_logit_scale, False, 0.0, 1e-7, self.p, self.raw_distance, 0.0, 1.0)
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
    ('mean' / 'sum') form.  Still one launch (``vlsa_surv_objective_terms``) up to 4096 samples; above, the per-sample launch, the two
    of SurvT2I and torch adds.  With the defaults the object is what it was and issues ``vlsa_surv_objective``."""

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
        self._default = converter == "softmax" and weight_t2i == 0       # (weight_mle is 0 here): today's launches, verbatim

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

    def _forward_terms(self, raw_pred, t, e, ls, is_log):
        if isinstance(ls, torch.Tensor) and raw_pred.is_cuda and raw_pred.dim() == 2 and raw_pred.shape[0] <= 4096:
            return _LaunchFn.apply(raw_pred, lambda x: _launch_objective_terms(x, t, e, ls, is_log, self._spec()))
        if is_log:
            ls = ls.detach().exp() if isinstance(ls, torch.Tensor) else float(torch.tensor(ls).exp())
        conv, family, alpha, eps, p, raw, w_main, w_emd, w_t2i, t2i_loss, t2i_reduction = self._spec()
        loss = _LaunchFn.apply(raw_pred, lambda x: _terms_rows(x, t, e, ls, conv, family, alpha, eps, p, raw, w_main, w_emd)).mean()
        if w_t2i != 0:
            loss = loss + _LaunchFn.apply(raw_pred, lambda x: _launch_t2i(x, t, e, ls, False, t2i_loss, t2i_reduction, w_t2i))
        return loss

    def forward(self, raw_pred, t, e=None, cur_logit_scale=10.0, log_logit_scale=None):
        """cur_logit_scale: exp(logit_scale) as the handler passes it (``net.get_logit_scale()``); log_logit_scale: the raw parameter
        instead (exponentiated inside the launch: one kernel less per step; no gradient flows into it either way -- the reference detaches it)."""
        if e is None:
            t, e = t[:, 0], t[:, 1]
        ls, is_log = (log_logit_scale, True) if log_logit_scale is not None else (cur_logit_scale, False)
        if not self._default:
            return self._forward_terms(raw_pred, t, e, ls, is_log)
        if isinstance(ls, torch.Tensor) and raw_pred.is_cuda and raw_pred.dim() == 2 and raw_pred.shape[0] <= 4096:
            return _SurvObjectiveFn.apply(raw_pred, t, e, ls, is_log, self.alpha, self.eps, self.p, self.raw, self.w1, self.w2)
        if is_log:
            ls = ls.detach().exp() if isinstance(ls, torch.Tensor) else float(torch.tensor(ls).exp())
        loss = _SurvLossFn.apply(raw_pred, t, e, ls, True, self.alpha, self.eps, self.p, self.raw, self.w1, self.w2)
        return loss.mean()

    def value_and_grad(self, raw_pred, t, e=None, log_logit_scale=None):
        """(objective, d objective / d raw_pred) from the one launch, outside autograd -- for a caller that owns the step and starts the
        backward pass itself with ``raw_pred.backward(grad)`` (``vlsa_amd.train_step.TrainStep``): ``loss.backward()`` costs two more
        launches (the ones_like seed and its product with the saved gradient), ~10 us of a graph-replayed step.  [B <= 4096, K] logits
        on the GPU, the raw (log) logit scale as a tensor."""
        if e is None:
            t, e = t[:, 0], t[:, 1]
        if not self._default:
            return self._value_and_grad_terms(raw_pred, t, e, log_logit_scale)
        lib = nat.load()
        x = raw_pred.detach().float().contiguous()
        _need_gpu(x)
        B, K = x.shape
        t = t.reshape(-1).to(device=x.device, dtype=torch.int64).contiguous()
        e = e.reshape(-1).to(device=x.device, dtype=torch.float32).contiguous()
        if t.numel() != B or e.numel() != B:
            raise ValueError("t and e must hold one entry per sample")
        ls = log_logit_scale.detach().to(device=x.device, dtype=torch.float32).reshape(1).contiguous()
        out = torch.empty(1 + B * K, dtype=torch.float32, device=x.device)
        g = out[1:].view(B, K)
        nat.check(lib.vlsa_surv_objective(_p(x), _p(t), _p(e), B, K, 1, _p(ls), 1, float(self.alpha), float(self.eps), int(self.p),
                                          int(self.raw), float(self.w1), float(self.w2), _p(out), _p(g), _stream()), "vlsa_surv_objective")
        return out[0], g

    def _value_and_grad_terms(self, raw_pred, t, e, log_logit_scale):
        """``value_and_grad`` of the other objectives: the one launch up to 4096 samples, else the launches of the autograd route"""
        if raw_pred.shape[0] <= 4096:
            return _launch_objective_terms(raw_pred, t, e, log_logit_scale, True, self._spec())
        conv, family, alpha, eps, p, raw, w_main, w_emd, w_t2i, t2i_loss, t2i_reduction = self._spec()
        rows, g = _terms_rows(raw_pred, t, e, log_logit_scale.detach().exp(), conv, family, alpha, eps, p, raw, w_main, w_emd)
        value, g = rows.mean(), g / g.shape[0]
        if w_t2i != 0:
            v2, g2 = _launch_t2i(raw_pred, t, e, log_logit_scale, True, t2i_loss, t2i_reduction, w_t2i)
            value, g = value + v2, g + g2
        return value, g
