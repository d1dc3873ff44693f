#!/usr/bin/env python
"""Fixtures of the handler's objectives beyond SurvIFMLE + SurvEMD: tests/golden/objective_<case>.npz (container only: imports the
reference; the cases and their inputs are tests/objective_cases.py FIXTURES; one file per family and shape holds its four
(alpha, reduction) variants, the per-variant entries as ``<variant>/<name>``).

Each holds the fp32 logits, t, e, the logit scale and the weights, and the REFERENCE's own results with its code fed float64:
  - hazard family: SurvMLE and SurvEMD on sigmoid(raw), SurvT2I('CL') on raw;
    incidence family: SurvIFMLE and SurvEMD on softmax(raw), SurvT2I('KL') on raw -- every term ('mean'-reduced per-sample terms), the
    total as calc_objective_loss weights it (runner/vlsa_handler.py:241-258) and its autograd gradient w.r.t. the raw logits;
  - ``NLLSurv_Evaluator(type, backend='none').compute`` with those loss objects as ``kws_ext_loss``: its dict in its key order.
A batch without a counted SurvT2I bin (``t2i_slots`` = 0) makes the reference return the float 0.0, on which its evaluator's ``.item()``
fails: the term is then stored as 0 and left out of the evaluator's run.

    python tests/golden/make_golden_objectives.py
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

import _ref_import

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import objective_cases as C  # noqa: E402


def _f64(v):
    return np.float64(v.detach() if torch.is_tensor(v) else v)


def main():
    _ref_import.import_reference()
    from eval.evaluator_surv import NLLSurv_Evaluator
    from loss.loss_surv import SurvIFMLE, SurvMLE
    from loss.loss_surv_ext import SurvEMD, SurvT2I
    files = {}
    for c in C.FIXTURES:
        i = C.case_inputs(c)
        hazard = c.family == "hazard"
        main_name = "SurvMLE" if hazard else "SurvIFMLE"
        with contextlib.redirect_stdout(io.StringIO()):
            losses = {main_name: (SurvMLE if hazard else SurvIFMLE)(alpha=c.alpha, eps=C.EPS), "SurvEMD": SurvEMD(p=c.p, raw_distance=c.raw),
                      "SurvT2I": SurvT2I(loss=c.t2i_loss, reduction=c.t2i_reduction)}
            ev = NLLSurv_Evaluator(c.family, backend="none")
        weight = {main_name: c.w_main, "SurvEMD": c.w_emd, "SurvT2I": c.w_t2i}
        ls = torch.tensor(float(np.float32(C.LOGIT_SCALE)), dtype=torch.float64)
        raw = i.logits.double().requires_grad_(True)
        t, e = i.t.view(-1, 1), i.e.double().view(-1, 1)
        y_hat = torch.sigmoid(raw) if hazard else torch.softmax(raw, dim=-1)
        terms = {main_name: losses[main_name](y_hat, t, e), "SurvEMD": losses["SurvEMD"](y_hat, t, e, ls),
                 "SurvT2I": losses["SurvT2I"](raw, t, e, ls)}
        slots = C.t2i_value(raw.detach(), i.t, i.e, float(ls), c.t2i_loss, c.t2i_reduction)[1]
        assert (slots == 0) == isinstance(terms["SurvT2I"], float)
        total = sum(weight[n] * terms[n] for n in terms)
        (grad,) = torch.autograd.grad(total, raw)
        shared = dict(family=np.array(c.family), logits=i.logits.numpy(), t=i.t.numpy().astype(np.int64), e=i.e.numpy().astype(np.float32),
                      logit_scale=np.float32(C.LOGIT_SCALE), eps=np.float64(C.EPS), p=np.int64(c.p), raw_distance=np.bool_(c.raw),
                      t2i_loss=np.array(c.t2i_loss), w_main=np.float64(c.w_main), w_emd=np.float64(c.w_emd), w_t2i=np.float64(c.w_t2i),
                      t2i_slots=np.int64(slots))
        out = dict(alpha=np.float64(c.alpha), t2i_reduction=np.array(c.t2i_reduction), ref64_main=_f64(terms[main_name]),
                   ref64_emd=_f64(terms["SurvEMD"]), ref64_t2i=_f64(terms["SurvT2I"]), ref64_total=_f64(total),
                   ref64_grad=grad.numpy().astype(np.float64))
        # the evaluator, as the handler calls it after a pass
        ext = {n: f for n, f in losses.items() if not (n == "SurvT2I" and slots == 0)}
        metrics = ["c_index", "loss", "loss_mle", "loss_mle_org"] if bool(i.e.any()) and c.B >= 2 else ["loss", "loss_mle", "loss_mle_org"]
        y = torch.stack([i.t.double(), i.e.double()], dim=1)
        res = ev.compute({"y": y, "y_hat": y_hat.detach(), "raw_y_hat": raw.detach(), "uid": None}, metrics, kws_ext_loss=ext,
                         loss_weight=weight, logit_scale=ls)
        shared["eval_keys"] = np.array(list(res))
        for k, v in res.items():
            out["eval_" + k] = np.float64(v)
        entry = files.setdefault(C.fixture_file(c), shared)          # (the shared entries are the same for the four variants of a file)
        assert all(np.array_equal(entry[k], v) for k, v in shared.items())
        entry.update({f"{C.variant(c)}/{k}": v for k, v in out.items()})
        print(f"{c.name}: slots {slots}, total {float(total):.12g}, " + ", ".join(f"{k}={float(v):.10g}" for k, v in res.items()))
    for name, entries in files.items():
        np.savez_compressed(os.path.join(HERE, name), **entries)


if __name__ == "__main__":
    main()
