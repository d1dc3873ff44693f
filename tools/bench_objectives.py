"""The handler's objectives beyond SurvIFMLE + SurvEMD: us per call of the ONE launch ``vlsa_surv_objective_terms`` (value and gradient:
``SurvObjective.value_and_grad``) against the reference-shaped torch sequence on the same device -- converter, per-sample likelihood
term, SurvEMD with a label loop over the batch, SurvT2I as a Python loop over the bins with two host synchronisations per bin, then
``autograd.grad``.

Shapes B x K: 32 x 4 and 32 x 12 (cfg_vlsa_conch.yaml's batch and bin counts), both families: hazard = SurvMLE + SurvEMD + 0.5 SurvT2I('CL')
behind the sigmoid, incidence = SurvIFMLE + SurvEMD + 0.5 SurvT2I('KL') behind the softmax.  Timing: wall clock around 20 back-to-back
calls with a device synchronisation before and after, divided by 20 (one launch alone is shorter than the clock's noise); 5 warm-up
rounds per route, then 20 such samples per route, the routes taking turns sample by sample in one process; the median of the 20.  The
whole comparison is repeated 3 times: ``us`` is the median of the three medians, ``spread`` their minimum and maximum.  Prints one JSON
line per shape and family, with both routes' objective.  Information, not a gate."""
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vlsa_amd.losses import SurvObjective  # noqa: E402

SHAPES = [(32, 4), (32, 12)]
WARMUP, INNER, CALLS, REPEATS = 5, 20, 20, 3
LOG_LOGIT_SCALE, EPS, W_T2I = 4.0309, 1e-7, 0.5


def torch_objective(raw, t, e, ls, family, t2i_loss):
    """the handler's calc_objective_loss written out in torch ops the way the reference's loss objects run them"""
    B, K = raw.shape
    tl, c = t.view(B, 1), 1.0 - e.view(B, 1)
    if family == "hazard":
        y = torch.sigmoid(raw)
        sp = torch.cat([torch.ones_like(c), torch.cumprod(1 - y, dim=1)], 1)
        unc = -(1 - c) * (torch.log(sp.gather(1, tl).clamp(min=EPS)) + torch.log(y.gather(1, tl).clamp(min=EPS)))
        cen = -c * torch.log(sp.gather(1, tl + 1).clamp(min=EPS))
    else:
        y = torch.softmax(raw, dim=-1)
        unc = -(1 - c) * torch.log(y.gather(1, tl).clamp(min=EPS))
        cen = -c * torch.log((1 - torch.cumsum(y, dim=1).gather(1, tl)).clamp(min=EPS))
    loss = (cen + unc).mean()
    # the label SurvEMD and SurvT2I share: a one at t, and ones behind it for a censored sample -- filled in sample by sample on the host's word
    ei = e.view(B, 1).long()
    target = torch.zeros(B, K, device=raw.device, dtype=torch.long)
    target[torch.arange(B, device=raw.device), t] = 1
    for i in range(B):
        first = int(t[i]) + 1
        if first < K:
            target[i, first:] += 1 - ei[i, 0]
    pred = (1 - ei) * ((1 - target) * y + target * ls) + ei * y
    d = torch.cumsum(torch.softmax(pred, dim=-1), dim=-1) - torch.cumsum(torch.softmax((2 * target - 1) * ls, dim=-1), dim=-1)
    loss = loss + (d ** 2).sum(dim=-1).mean()
    # SurvT2I: bin by bin over the samples that take part, two host reads per bin
    part = ~((target == 1) & (ei == 0))
    total, slots = 0.0, 0
    for k in range(K):
        rows = part[:, k]
        if not bool(rows.any()):
            continue
        tk = target[rows, k].to(raw.dtype)
        if float(tk.sum()) == 0:
            continue
        lp = torch.log_softmax(raw[rows, k], dim=0)
        if t2i_loss == "CL":
            cur = -(tk * lp).sum() / tk.sum()
        else:
            td = torch.softmax((2 * tk - 1) * ls, dim=0)
            cur = (torch.xlogy(td, td) - td * lp).sum()
        total, slots = total + cur, slots + 1
    if slots:
        loss = loss + W_T2I * total / slots
    return loss


def sample(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(INNER):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / INNER, out


def main():
    dev = torch.device("cuda", 0)
    ls_log = torch.tensor(LOG_LOGIT_SCALE, device=dev)
    ls = ls_log.exp()
    for B, K in SHAPES:
        g = torch.Generator().manual_seed(100 * K + B)
        raw = (2.0 * torch.randn(B, K, generator=g)).to(dev)
        t = torch.randint(0, K - 1, (B,), generator=g).to(dev)
        e = (torch.rand(B, generator=g) < 0.45).float().to(dev)
        for family, t2i_loss in (("hazard", "CL"), ("incidence", "KL")):
            hazard = family == "hazard"
            obj = SurvObjective(weight_ifmle=0.0 if hazard else 1.0, weight_mle=1.0 if hazard else 0.0, weight_emd=1.0, weight_t2i=W_T2I,
                                converter="sigmoid" if hazard else "softmax", t2i_loss=t2i_loss)

            def launch():
                return obj.value_and_grad(raw, t, e, log_logit_scale=ls_log)

            def torch_sequence():
                x = raw.detach().requires_grad_(True)
                loss = torch_objective(x, t, e, ls, family, t2i_loss)
                return loss.detach(), torch.autograd.grad(loss, x)[0]

            routes = {"one_launch": launch, "torch_sequence": torch_sequence}
            outs = {}
            for name, fn in routes.items():
                for _ in range(WARMUP):
                    outs[name] = sample(fn)[1]
            meds = {name: [] for name in routes}
            for _ in range(REPEATS):
                ts = {name: [] for name in routes}
                for _ in range(CALLS):
                    for name, fn in routes.items():
                        ts[name].append(sample(fn)[0])
                for name in routes:
                    meds[name].append(statistics.median(ts[name]))
            dv = abs(outs["one_launch"][0].item() - outs["torch_sequence"][0].item())
            dg = (outs["one_launch"][1] - outs["torch_sequence"][1]).abs().max().item()
            line = {"op": "surv_objective_terms", "family": family, "t2i": t2i_loss, "B": B, "K": K, "value_diff": dv, "grad_diff": dg}
            for name in routes:
                line[name] = {"us": round(statistics.median(meds[name]), 1), "spread": [round(min(meds[name]), 1), round(max(meds[name]), 1)],
                              "objective": outs[name][0].item()}
            assert math.isfinite(dv) and dv < 1e-3 and dg < 1e-3, line        # the two routes time the same objective
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a GPU: no timing without one"
    main()
