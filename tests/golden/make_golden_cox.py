#!/usr/bin/env python
"""Fixtures of the continuous survival heads: the objective, tests/golden/cox_objective_b<B>_<times>.npz, and the evaluators' pieces on a
split, tests/golden/cox_split_m<M>_<times>.npz (see split_fixtures below).  Container only: imports the reference.  The objective's cases and their inputs are tests/cox_cases.py
FIXTURES; one file per batch size and time variant holds its l1 and l2 variants, the per-variant entries as ``<norm>/<name>``.

Each holds t, e, the options and the weights, per variant the fp32 prediction (the input rule of cox_cases.py moves l1's), and the
REFERENCE's own results with its code fed float64: ``SurvPLE()`` (its B x B Python loop included), ``rank_loss``, ``recon_loss`` and
``MSE_loss`` of loss/loss_surv.py on a [B, 1] prediction, every term, the weighted total and its autograd gradient w.r.t. the prediction.
The three functions get t and e as the [B, 1] columns ``calc_objective_loss`` passes (runner/sa_handler.py:172-180); ``SurvPLE`` gets
them as [B] vectors, the form its docstring describes: on [B, 1] columns its product ``(theta - log ...) * E.float()`` broadcasts a [B]
vector against a [B, 1] column into [B, B], and the mean becomes mean(theta - log D) * mean(e) -- not the partial likelihood
(INTEGRATION.md, section 7).  A batch without a rank pair makes the reference return ``Tensor([0.])``
outside the graph: the term is stored as 0 and adds no gradient.  The number of rank pairs is counted here from the labels.

    python tests/golden/make_golden_cox.py
"""
import os
import sys

import numpy as np
import torch

import _ref_import

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cox_cases as C  # noqa: E402


def main():
    _ref_import.import_reference()
    from loss.loss_surv import MSE_loss, SurvPLE, rank_loss, recon_loss
    files = {}
    for c in C.FIXTURES:
        i = C.case_inputs(c)
        pred = i.pred.double().view(-1, 1).requires_grad_(True)
        t, e = i.t.double().view(-1, 1), i.e.double().view(-1, 1)
        terms = {"SurvPLE": SurvPLE()(pred, t.view(-1), e.view(-1)),
                 "rank_loss": rank_loss(pred, t, e, gamma=c.rank_gamma, norm=c.rank_norm, add_weight=False),
                 "recon_loss": recon_loss(pred, t, e, alpha=c.recon_alpha, gamma=c.recon_gamma, norm=c.recon_norm),
                 "MSE_loss": MSE_loss(pred, t, e, include_censored=c.mse_censored)}
        weight = {"SurvPLE": c.w_ple, "rank_loss": c.w_rank, "recon_loss": c.w_recon, "MSE_loss": c.w_mse}
        pairs = int(((i.t.view(-1, 1) < i.t.view(1, -1)) & (i.e.view(-1, 1) == 1)).sum())
        assert (pairs == 0) == (not terms["rank_loss"].requires_grad)
        total = sum(weight[n] * terms[n].reshape(()) for n in terms)
        (grad,) = torch.autograd.grad(total, pred)
        shared = dict(t=i.t.numpy(), e=i.e.numpy(), rank_pairs=np.int64(pairs), rank_gamma=np.float64(c.rank_gamma),
                      recon_alpha=np.float64(c.recon_alpha), recon_gamma=np.float64(c.recon_gamma), mse_censored=np.bool_(c.mse_censored),
                      weights=np.array([c.w_ple, c.w_rank, c.w_recon, c.w_mse], dtype=np.float64))
        out = dict(norm=np.array(c.rank_norm), pred=i.pred.numpy(), ref64_ple=np.float64(terms["SurvPLE"].detach()),
                   ref64_rank=np.float64(terms["rank_loss"].detach().reshape(())), ref64_recon=np.float64(terms["recon_loss"].detach()),
                   ref64_mse=np.float64(terms["MSE_loss"].detach()), ref64_total=np.float64(total.detach()),
                   ref64_grad=grad.reshape(-1).numpy().astype(np.float64))
        entry = files.setdefault(C.fixture_file(c), shared)       # (the shared entries are the same for the variants of a file)
        assert all(np.array_equal(entry[k], v) for k, v in shared.items())
        entry.update({f"{c.rank_norm}/{k}": v for k, v in out.items()})
        print(f"{c.name}: pairs {pairs}, " + ", ".join(f"{n}={float(v):.10g}" for n, v in terms.items()) + f", total {float(total):.12g}")
    for name, entries in files.items():
        np.savez_compressed(os.path.join(HERE, name), **entries)
    split_fixtures()


def split_fixtures():
    """tests/golden/cox_split_m<M>_<times>.npz: the evaluators' pieces on cox_cases.split_inputs, the reference's code fed float64.
    ``CoxSurv_Evaluator.compute`` itself is NOT run: its constructor needs a MetaSurvData table and its 'train' pass the SurvivalEVAL
    backend; stored instead are the calls it makes -- ``concordance_index(..., type_pred='hazard_ratio')`` with the five counts of
    ``concordance_index_censored(e, t, -y_hat)`` behind it, ``SurvPLE()(y_hat, t, e)`` on vectors, ``BreslowEstimator().fit`` /
    ``get_survival_function(ret_ndarray=True)`` (times, cumulative baseline hazard, and three rows of the [M, U] curves: vectors only).
    ``RegSurv_Evaluator(end_time=12).compute`` is run for its eight computable metrics; its ``c_index`` raises AssertionError in the
    reference (asserted here), so the counts of the call behind the assertion are stored."""
    from eval.cindex import concordance_index, concordance_index_censored
    from eval.evaluator_surv import RegSurv_Evaluator
    from eval.utils_coxph import BreslowEstimator
    from loss.loss_surv import SurvPLE
    for M in C.SPLIT_SHAPES:
        for times in C.TIMES:
            i = C.split_inputs(M, times)
            y_hat, reg_pred, t, e = i.y_hat.double(), i.reg_pred.double(), i.t.double(), i.e.double()
            y = torch.stack([t, e], dim=1)
            out = dict(y_hat=i.y_hat.numpy(), reg_pred=i.reg_pred.numpy(), t=i.t.numpy(), e=i.e.numpy(), end_time=np.float64(C.END_TIME))
            out["cox_c_index"] = np.float64(concordance_index(y.numpy(), y_hat.view(-1, 1).numpy(), type_pred="hazard_ratio"))
            for key, pred in (("cox", y_hat), ("reg", reg_pred)):
                five = concordance_index_censored(e.numpy().astype(bool), t.numpy(), -pred.numpy(), tied_tol=1e-8)
                out[key + "_cindex"] = np.float64(five[0])
                out[key + "_counts"] = np.array(five[1:], dtype=np.int64)       # concordant, discordant, tied_risk, tied_time
            assert out["cox_c_index"] == out["cox_cindex"]
            out["loss_ple"] = np.float64(SurvPLE()(y_hat, t, e))
            est = BreslowEstimator().fit(y_hat.numpy(), e.numpy().astype(bool), t.numpy())
            times_u, surv = est.get_survival_function(y_hat.numpy(), ret_ndarray=True)
            rows = np.array(sorted({0, M // 2, M - 1}), dtype=np.int64)
            out.update(time_points=np.asarray(times_u, dtype=np.float64), cum_hazard=np.asarray(est.cum_baseline_hazard_.y, dtype=np.float64),
                       survival_rows=rows, survival_hat_rows=np.asarray(surv, dtype=np.float64)[rows])
            ev = RegSurv_Evaluator(end_time=C.END_TIME)
            data = {"y": y, "y_hat": reg_pred.view(-1, 1), "uid": None, "name": "test"}
            res = ev.compute(data, list(C.REG_METRICS))
            for k, v in res.items():
                out["reg_" + k] = np.float64(v)
            try:
                ev.compute(data, ["c_index"])
                raise SystemExit("RegSurv_Evaluator._c_index ran: the finding of INTEGRATION.md section 7 no longer holds")
            except AssertionError:
                pass
            out["reg_rank_pairs"] = np.int64(((i.t.view(-1, 1) < i.t.view(1, -1)) & (i.e.view(-1, 1) == 1)).sum())
            np.savez_compressed(os.path.join(HERE, C.split_fixture_file(M, times)), **out)
            print(f"split m{M}-{times}: C {float(out['cox_cindex']):.6f} / {float(out['reg_cindex']):.6f}, loss_ple {float(out['loss_ple']):.8g}, "
                  f"U {len(times_u)}, " + ", ".join(f"{k}={float(v):.6g}" for k, v in res.items()))


if __name__ == "__main__":
    main()
