#!/usr/bin/env python
"""Fixtures of the device-side survival evaluator: tests/golden/surv_eval_<case>.npz (container only: imports the reference).

Each holds the fp32 logits, t, e, the logit scale and the loss weights, and the REFERENCE's own results with its code fed float64:
``NLLSurv_Evaluator(type, backend='none').compute`` on ``converter(raw.double())`` with reference SurvIFMLE / SurvEMD instances as
``kws_ext_loss`` (incidence), and the 5-tuple of ``concordance_index_censored`` on the float64 risk; plus the reference's plain fp32
run of the same metrics (``ref32_*``, for information).

The seed of a case is redrawn until (tests/test_surv_eval_cpu.py asserts both)
  - every non-zero gap between sorted float64 risks is >= 1e-6 (100 x tied_tol): exact ties come only from bit-identical rows, so no
    pair count hangs on rounding;
  - no censored sample sits in the last bin, where the reference takes log(clamp(1 - 1, eps)), decided by the last ulp.  The one case
    named ``lastbin_incidence`` holds nothing else and is checked against the bound -log(1e-7) <= loss <= -log(1e-7) + 1e-6.

    python tests/golden/make_golden_surv_eval.py
"""
import contextlib
import io
import math
import os

import numpy as np
import torch

import _ref_import

HERE = os.path.dirname(os.path.abspath(__file__))
LOGIT_SCALE = np.float32(math.exp(4.0309))          # exp of the shipped checkpoint's logit scale
MIN_GAP = 1e-6
# (name, M, K, flags): 'dup' = bit-identical logit rows (exact risk ties) under different labels, 'all_events', 'one_event'
SHAPES = [("m2_k2", 2, 2, ("one_event",)), ("m3_k4", 3, 4, ("all_events",)), ("m65_k4", 65, 4, ("dup", "one_event")),
          ("m257_k12", 257, 12, ("dup",)), ("m1025_k4", 1025, 4, ("dup",))]
EXT = {"m2_k2": (0.0, 2, True), "m3_k4": (0.25, 1, True), "m65_k4": (0.5, 2, False), "m257_k12": (0.25, 2, True),
       "m1025_k4": (0.0, 2, True)}           # (alpha of the ext SurvIFMLE, p and raw_distance of the ext SurvEMD)
W_IFMLE, W_EMD = 1.0, 0.5


def draw(M, K, flags, seed):
    g = torch.Generator().manual_seed(seed)
    raw = (1.5 * torch.randn(M, K, generator=g)).float()
    t = torch.randint(0, K, (M,), generator=g)
    e = (torch.rand(M, generator=g) < 0.6).float()
    if "dup" in flags:                                  # copies of a row a few places on, and a run of three
        for a, b in [(3, 5), (3, M // 3), (M // 2, M // 2 + 1), (M - 2, 7)]:
            raw[b] = raw[a]
    if "all_events" in flags:
        e[:] = 1.0
    if "one_event" in flags:
        e[:] = 0.0
        e[0] = 1.0
        t[0] = 0
    cen_last = (e == 0) & (t == K - 1)
    t[cen_last] = K - 2                                  # (tied times with mixed events come with the bins)
    return raw, t, e


def reference_run(ns, ptype, raw, t, e, ext, dtype):
    """the reference's evaluator and C tuple on inputs of `dtype`"""
    conv = (lambda x: torch.softmax(x, dim=-1)) if ptype == "incidence" else torch.sigmoid
    y_hat = conv(raw.to(dtype))
    y = torch.stack([t.to(dtype), e.to(dtype)], dim=1)
    with contextlib.redirect_stdout(io.StringIO()):
        ev = ns.NLLSurv_Evaluator(ptype, backend="none")
        losses = None
        if ext is not None:
            losses = {"SurvIFMLE": ns.SurvIFMLE(alpha=ext[0], eps=1e-7), "SurvEMD": ns.SurvEMD(p=ext[1], raw_distance=ext[2])}
    has_pairs = bool(e.any()) and len(t) >= 2
    metrics = ["c_index", "loss", "loss_mle", "loss_mle_org"] if has_pairs else ["loss", "loss_mle", "loss_mle_org"]
    kws = dict(loss_weight={"SurvIFMLE": W_IFMLE, "SurvEMD": W_EMD}, logit_scale=torch.tensor(float(LOGIT_SCALE), dtype=dtype)) if losses else {}
    res = ev.compute({"y": y, "y_hat": y_hat, "uid": None}, metrics, kws_ext_loss=losses, **kws)
    yp = y_hat.numpy()
    surv = 1.0 - np.cumsum(yp, axis=1) if ptype == "incidence" else np.cumprod(1.0 - yp, axis=1)      # eval/cindex.py:36-43
    risk = np.sum(surv, axis=1)
    tup = ns.concordance_index_censored(e.numpy().astype(np.bool_), t.to(dtype).numpy(), -risk, tied_tol=1e-08) if has_pairs else None
    return res, tup, -risk


def draw_ok(ptype, raw, t, e):
    """the two conditions on a draw that the docstring states, and at least one comparable pair"""
    y_hat = (torch.softmax(raw.double(), dim=-1) if ptype == "incidence" else torch.sigmoid(raw.double())).numpy()
    surv = 1.0 - np.cumsum(y_hat, axis=1) if ptype == "incidence" else np.cumprod(1.0 - y_hat, axis=1)
    d = np.diff(np.sort(np.sum(surv, axis=1)))
    tn, ev = t.numpy(), e.numpy() != 0
    comparable = ev[:, None] & ((tn[None, :] > tn[:, None]) | ((tn[None, :] == tn[:, None]) & ~ev[None, :]))
    return bool(np.all((d == 0) | (d >= MIN_GAP))) and bool(comparable.any()) and not bool((~ev & (tn == raw.shape[1] - 1)).any())


def save(ns, name, ptype, raw, t, e, ext, seed):
    res64, tup64, est64 = reference_run(ns, ptype, raw, t, e, ext, torch.float64)
    res32, tup32, _ = reference_run(ns, ptype, raw, t, e, ext, torch.float32)
    out = dict(prediction_type=np.array(ptype), seed=np.int64(seed), raw=raw.numpy(), t=t.numpy().astype(np.int64), e=e.numpy().astype(np.float32),
               ref64_est=np.asarray(est64, dtype=np.float64))
    if ext is not None:
        out.update(logit_scale=LOGIT_SCALE, w_ifmle=np.float64(W_IFMLE), w_emd=np.float64(W_EMD), ext_alpha=np.float64(ext[0]),
                   ext_eps=np.float64(1e-7), p=np.int64(ext[1]), raw_distance=np.bool_(ext[2]))
    for tag, res, tup in (("ref64", res64, tup64), ("ref32", res32, tup32)):
        for k, v in res.items():
            out[f"{tag}_{k}"] = np.float64(v)
        if tup is not None:
            c, con, dis, tied_risk, tied_time = tup
            out[f"{tag}_cindex_censored"] = np.float64(c)
            out[f"{tag}_counts"] = np.array([con, dis, tied_risk, tied_time, con + dis + tied_risk], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, f"surv_eval_{name}.npz"), **out)
    print(f"{name}: seed {seed}, " + ", ".join(f"{k}={float(v):.12g}" for k, v in res64.items())
          + (f", counts {out['ref64_counts'].tolist()}, fp32 C {res32['c_index']:.12g}" if tup64 is not None else ""))


def main():
    _ref_import.import_reference()
    import types
    from eval.cindex import concordance_index_censored
    from eval.evaluator_surv import NLLSurv_Evaluator
    from loss.loss_surv import SurvIFMLE
    from loss.loss_surv_ext import SurvEMD
    ns = types.SimpleNamespace(NLLSurv_Evaluator=NLLSurv_Evaluator, concordance_index_censored=concordance_index_censored,
                               SurvIFMLE=SurvIFMLE, SurvEMD=SurvEMD)
    for ci, (shape, M, K, flags) in enumerate(SHAPES):
        for pi, ptype in enumerate(("incidence", "hazard")):
            seed = 7000 + 100 * ci + 50 * pi
            while True:
                raw, t, e = draw(M, K, flags, seed)
                if draw_ok(ptype, raw, t, e):
                    break
                seed += 1
            save(ns, f"{shape}_{ptype}", ptype, raw, t, e, EXT[shape] if ptype == "incidence" else None, seed)
    # censored samples in the last bin and nothing else (no event: the loss metrics only)
    raw = (1.5 * torch.randn(4, 4, generator=torch.Generator().manual_seed(7900))).float()
    save(ns, "lastbin_incidence", "incidence", raw, torch.full((4,), 3), torch.zeros(4), None, 7900)


if __name__ == "__main__":
    main()
