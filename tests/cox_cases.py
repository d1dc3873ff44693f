"""Cases and float64 truth of the continuous survival heads' objective (vlsa_amd/csrc/surv_pairs.hip): SurvPLE, rank_loss, recon_loss and
MSE_loss of loss/loss_surv.py on a one-column prediction, shared by tests/test_cox_cases_cpu.py (the restatement against the reference's
own float64 results in tests/golden/cox_*.npz, the input conditions, the gates) and tests/test_gpu_cox_objective.py (the kernel).
CPU only: torch and tests/objective_cases.py (BAND, MAX_ALTERED, the error measures)."""
import collections
import functools
import glob
import os

import numpy as np
import torch

from objective_cases import BAND, MAX_ALTERED, rel_grad, rel_value  # noqa: F401  (the tests read them from here)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- what the launch branches on (tests/test_cox_cases_cpu.py::test_dispatch_constants_match_the_source reads them from the code)
WAVE = 64                # the workgroup is B rounded up to whole waves ...
THREADS = 1024           # ... up to kPairObjThreads; above, a thread owns up to kPairObjOwned = 4 samples, thread i % 1024 owns sample i
OWNED = 4
MAX_B = 4096             # kPairObjMaxB = VLSA_PAIR_MAX_B: a larger batch is VLSA_EUNSUPPORTED for the one launch
CAP = 10.0               # SurvPLE's CONSTANT
BATCH_EDGES = sorted({1, 2, 3, 130} | {g + d for g in (WAVE, THREADS) for d in (-1, 0, 1)} | {2 * THREADS + 1, MAX_B - 1, MAX_B})
REFUSED_B = MAX_B + 1      # refused by vlsa_surv_pair_objective itself; SurvPairObjective takes its split route there
# l1 terms are drawn up to this batch.  A rank pair sits inside the band around its kink (below) with probability ~1e-3; at B = 130 that
# is ~5 % of the samples, which the input rule redraws; at B >= 1023 every sample has such a partner and no normal draw can satisfy the
# rule.  The larger batches of the grid therefore run the l2 forms, which have no kink; L1_LARGE (below) adds the l1 forms there.
L1_MAX_B = 130

# ---- the gates: 8 x the worst error of a plain fp32 evaluation of the same formulas on the CPU (truth(dtype=torch.float32): the
# reference's formulas, vectorised) against the float64 truth over every case below, rounded up to one significant digit.
# tests/test_cox_cases_cpu.py::test_gates_are_eight_times_the_fp32_restatement measures them and asserts that the restatement stays within
# an eighth of each.  Value: relative to max(1, |value|); gradient: relative to max(largest float64 entry, 1 / B).  Measured worst cases:
#   value    1.82e-7 (grid-b3-f32-mixed)
#   gradient 1.94e-7 (l1rank-b1025-f32-mixed-steps)
# The 1 / B floor is a definition, as in objective_cases.py: a batch whose float64 gradient vanishes owes nothing relative to it.
VALUE_RTOL = 2e-6
GRAD_RTOL = 2e-6

Case = collections.namedtuple("Case", "name B seed times censor w_ple w_rank w_recon w_mse rank_gamma rank_norm recon_alpha recon_gamma "
                                      "recon_norm mse_censored pred_kind")
TIMES = ("f32", "ties")                       # fp32 draws without ties; integer times in 0 .. 11 with many ties
CENSOR = ("mixed", "all-censored", "all-event", "no-pair")
WEIGHTS = (1.0, 0.7, 0.5, 0.3)                # SurvPLE, rank_loss, recon_loss, MSE_loss


def _case(prefix, B, times, censor="mixed", w=WEIGHTS, norm=None, rank_gamma=1.0, recon_alpha=0.3, recon_gamma=1.0, mse_censored=False, tag="",
          recon_norm=None, pred_kind="normal"):
    """norm: of rank_loss, and of recon_loss unless recon_norm names its own.  pred_kind 'steps': predictions on multiples of 4 (below)"""
    norm = norm or ("l1" if B <= L1_MAX_B else "l2")
    seed = SEEDS.get((prefix, B, times, censor, tag), 9000 + 10 * B + TIMES.index(times) + 100003 * CENSOR.index(censor))
    return Case(f"{prefix}-b{B}-{times}-{censor}{tag}", B, seed, times, censor, w[0], w[1], w[2], w[3], rank_gamma, norm, recon_alpha, recon_gamma,
                recon_norm or norm, mse_censored, pred_kind)


# seeds that had to be chosen so that the input rule alters at most MAX_ALTERED of a case's samples: the default seed serves every case
SEEDS = {}
GRID = [_case("grid", B, times) for B in BATCH_EDGES for times in TIMES]
CENSORED = [_case("cen", 33, times, censor) for times in TIMES for censor in CENSOR[1:]]
ONE_TERM = tuple(tuple(1.0 if k == j else 0.0 for k in range(4)) for j in range(4))
OPTIONS = [_case("opt", 33, times, w=w, norm=norm, rank_gamma=g, recon_alpha=a, recon_gamma=g, mse_censored=mc,
                 tag=f"-w{'/'.join(f'{v:g}' for v in w)}-{norm}-g{g:g}-a{a:g}-{'mc' if mc else 'me'}")
           for times in TIMES for w in ONE_TERM + ((0.0, 1.3, 0.7, 2.0),) for norm in ("l1", "l2") for (g, a, mc) in ((1.0, 0.0, False), (0.5, 0.3, True))]
# l1 past the batches normal draws allow.  recon_loss's kink is per sample, so the input rule holds at any size: recon l1 beside rank l2
# where a thread owns several samples (1025, 4096).  rank_loss l1 there needs predictions that keep EVERY pair off its kink: 'steps' draws
# them from the multiples of 4 in [-20, 20] (ties among predictions, seven values above the cap), so gamma + p_i - p_j is 1 + 4 k, at
# least 1 / 20 of the numbers added -- fifty bands away; recon_loss is left out of those (a time may sit next to a multiple of 4).
STEPS_WEIGHTS = (1.0, 0.7, 0.0, 0.3)
L1_LARGE = ([_case("l1recon", B, times, norm="l2", recon_norm="l1", tag="-rank-l2-recon-l1") for B in (THREADS + 1, MAX_B) for times in TIMES]
            + [_case("l1rank", B, times, w=STEPS_WEIGHTS, norm="l1", pred_kind="steps", tag="-steps") for B in (THREADS + 1, MAX_B) for times in TIMES])
CASES = GRID + CENSORED + OPTIONS + L1_LARGE
# the first batch past the one launch: SurvPairObjective takes the split launches (float64 pair sums) plus torch adds
SPLIT_ROUTE = ([_case("split", MAX_B + 1, times) for times in TIMES] + [_case("split", MAX_B + 1, "ties", w=(0.0, 1.0, 0.0, 0.0), tag="-rank")]
               + [_case("split", MAX_B + 1, "f32", norm="l2", recon_norm="l1", tag="-rank-l2-recon-l1"),
                  _case("split", MAX_B + 1, "ties", w=STEPS_WEIGHTS, norm="l1", pred_kind="steps", tag="-l1-steps")])
FIXTURE_SHAPES = (1, 5, 33, 130)
FIXTURES = [_case("fix", B, times, norm=norm, tag=f"-{norm}") for B in FIXTURE_SHAPES for times in TIMES for norm in ("l1", "l2")]


def ids(cases):
    return [c.name for c in cases]


def fixture_file(c):
    return f"cox_objective_b{c.B}_{c.times}.npz"


def load_fixture(c):
    """the fixture of ONE case: the shared entries, and the entries stored as `<norm>/<name>` under their name"""
    tag = c.rank_norm + "/"
    with np.load(os.path.join(GOLDEN, fixture_file(c)), allow_pickle=False) as z:
        out = {k: z[k] for k in z.files if "/" not in k}
        out.update({k[len(tag):]: z[k] for k in z.files if k.startswith(tag)})
    return out


def fixture_files():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "cox_objective_*.npz")))


# ---- inputs
Inputs = collections.namedtuple("Inputs", "pred t e changed")


def kink_distance(pred, t, e, c):
    """[B] float64: for each sample the smallest |x| / scale over the l1 kinks it takes part in with a non-zero weight -- x = pred - t
    of an event and gamma - (pred - t) of a censored sample (recon_loss), gamma + p_i - p_j of a pair with e_i == 1 and t_i < t_j, charged
    to both of its samples (rank_loss); scale = the largest magnitude among the numbers added.  inf where there is none."""
    p, tt, ee = pred.double(), t.double(), e.double()
    out = torch.full_like(p, float("inf"))
    if c.w_recon != 0 and c.recon_norm == "l1":
        d = p - tt
        scale = torch.maximum(p.abs(), tt.abs()).clamp(min=abs(c.recon_gamma))
        out = torch.minimum(out, torch.where(ee != 0, d.abs(), (c.recon_gamma - d).abs()) / scale)
    if c.w_rank != 0 and c.rank_norm == "l1":
        x = (c.rank_gamma + p.view(-1, 1) - p.view(1, -1)).abs()
        scale = torch.maximum(p.abs().view(-1, 1), p.abs().view(1, -1)).clamp(min=abs(c.rank_gamma))
        mask = (tt.view(-1, 1) < tt.view(1, -1)) & (ee.view(-1, 1) == 1)
        r = torch.where(mask, x / scale, torch.full_like(x, float("inf")))
        out = torch.minimum(out, torch.minimum(r.min(dim=1).values, r.min(dim=0).values))
    return out


def in_band(pred, t, e, c):
    return kink_distance(pred, t, e, c) < BAND


def _draw_pred(n, g):
    return torch.randn(n, generator=g) * 5.0


@functools.lru_cache(maxsize=None)
def case_inputs(c):
    """pred [B] fp32 = randn * 5 (about 2 % above SurvPLE's cap of 10; from four samples on, sample 0 sits ON the cap and sample 1 above
    it), t [B] fp32 -- a jittered shuffled grid over (0, 12), no ties, or integers in 0 .. 11 --, e [B] fp32 ~ Bernoulli(0.6) (40 %
    censored) or what `censor` says: 'no-pair' gives the event to the samples at the largest time only, so that no rank pair exists.  The input rule: a sample
    inside the band around an l1 kink (in_band) gets a new prediction.  `changed`: the samples it altered.  (Cached: read-only.)"""
    g = torch.Generator()
    g.manual_seed(c.seed)
    B = c.B
    pred = _draw_pred(B, g) if c.pred_kind == "normal" else 4.0 * torch.randint(-5, 6, (B,), generator=g).float()
    if c.times == "ties":
        t = torch.randint(0, 12, (B,), generator=g).float()
    else:
        # a shuffled grid over (0, 12) with a jitter of half a step: 4096 plain fp32 uniforms would collide
        t = (torch.randperm(B, generator=g).float() + 0.5 * torch.rand(B, generator=g)) * (12.0 / B)
        assert len(torch.unique(t)) == B
    e = (torch.rand(B, generator=g) < 0.6).float()
    if c.censor == "all-censored":
        e = torch.zeros(B)
    elif c.censor == "all-event":
        e = torch.ones(B)
    elif c.censor == "no-pair":
        e = (t == t.max()).float()
    fixed = torch.zeros(B, dtype=torch.bool)
    if B >= 4:
        pred[0], pred[1] = CAP, 12.5
        fixed[:2] = True
        if c.censor in ("mixed", "all-event"):
            e[0] = 1.0                      # an event ON the cap; among integer times away from recon_loss's kink at t = 10
            if c.times == "ties":
                t[0] = 3.0
    altered = torch.zeros(B, dtype=torch.bool)
    for _ in range(100):
        band = in_band(pred, t, e, c) & ~fixed      # (a rank pair is charged to both of its samples: the partner of a placed one moves)
        if not bool(band.any()):
            break
        altered |= band
        pred[band] = _draw_pred(int(band.sum()), g)
    assert not bool(in_band(pred, t, e, c).any()), f"{c.name}: the input rule did not converge"
    return Inputs(pred, t, e, int(altered.sum()))


# ---- exact kinks, each its own case and outside the input rule: name -> (pred, t, e), every number representable; gamma = 1
EDGES = {
    # recon_loss l1: |pred - t| at 0 for the event (derivative 0), a censored sample next to it
    "pred-equals-t": (torch.tensor([2.0, 3.5, 1.0]), torch.tensor([2.0, 1.0, 1.5]), torch.tensor([1.0, 1.0, 0.0])),
    # recon_loss: relu(gamma - (pred - t)) at 0 for the censored sample
    "gamma-minus-d-is-zero": (torch.tensor([3.0, 0.25, 4.0]), torch.tensor([2.0, 1.0, 6.0]), torch.tensor([0.0, 1.0, 0.0])),
    # rank_loss: relu(gamma + p_0 - p_1) at 0 for the pair (0, 1)
    "rank-pair-on-the-kink": (torch.tensor([1.0, 2.0, 0.5]), torch.tensor([1.0, 2.0, 3.0]), torch.tensor([1.0, 1.0, 0.0])),
    # SurvPLE: every prediction above the cap: theta = 10 for all, no gradient
    "all-above-the-cap": (torch.tensor([11.0, 40.0, 10.5]), torch.tensor([1.0, 2.0, 3.0]), torch.tensor([1.0, 0.0, 1.0])),
    # SurvPLE: far apart predictions, where the unshifted exp of the smaller ones underflows next to the largest
    "wide-spread": (torch.tensor([-60.0, 9.0, -3.0, -90.0]), torch.tensor([4.0, 1.0, 2.0, 3.0]), torch.tensor([1.0, 1.0, 0.0, 1.0])),
}
EDGE_CASE = _case("edge", 3, "f32", norm="l1")          # the options of every edge: all four terms, l1
EDGE_CASE_L2 = _case("edge", 3, "f32", norm="l2")


# ---- the float64 restatement
def ple_value(pred, t, e):
    """SurvPLE (loss/loss_surv.py:189-209) with the risk matrix as a broadcast comparison"""
    theta = torch.where(pred > CAP, torch.full_like(pred, CAP), pred)
    R = (t.view(1, -1) >= t.view(-1, 1)).to(pred.dtype)
    return -torch.mean((theta - torch.log(torch.sum(torch.exp(theta) * R, dim=1))) * e)


def rank_value(pred, t, e, gamma=1.0, norm="l1", fp32_weights=False):
    """(rank_loss, the number of pairs): loss/loss_surv.py:33-70 with add_weight = False, the exact mean over the pairs.  fp32_weights:
    the reference's own pair weights instead, which are fp32 whatever the prediction's dtype -- the sum times the 24-bit rounding of
    1 / n, within 6e-8 of the mean, relative; only the comparisons with the reference's float64 results ask for it.  No pair: a zero
    that carries the graph"""
    mask = (t.view(-1, 1) < t.view(1, -1)) & (e.view(-1, 1) == 1)
    n = int(mask.sum())
    if n == 0:
        return pred.sum() * 0.0, 0
    loss = torch.relu(gamma + pred.view(-1, 1) - pred.view(1, -1))
    if norm == "l2":
        loss = loss * loss
    m = mask.float() if fp32_weights else mask.to(pred.dtype)
    return (loss * (m / m.sum())).sum(), n


def recon_value(pred, t, e, alpha=0.0, gamma=1.0, norm="l1"):
    obs = e * torch.abs(pred - t)
    cen = (1 - e) * torch.relu(gamma - (pred - t))
    if norm == "l2":
        obs, cen = obs * obs, cen * cen
    return ((1.0 - alpha) * (obs + cen) + alpha * obs).mean()


def mse_value(pred, t, e, include_censored=False):
    loss = e * (pred - t) * (pred - t)
    if include_censored:
        loss = loss + (1 - e) * (pred - t) * (pred - t)
    return loss.mean()


Truth = collections.namedtuple("Truth", "ple rank recon mse pairs objective grad")


def truth(pred, t, e, c, dtype=torch.float64, fp32_weights=False):
    """the four terms, the pair count, objective = sum of weight * term over the terms with a weight, and d objective / d pred [B] by
    autograd, all in `dtype` (float64: the truth; float32: the plain fp32 restatement the gates are measured on)"""
    x = pred.detach().reshape(-1).to(dtype).requires_grad_(True)
    t, e = t.reshape(-1).to(dtype), e.reshape(-1).to(dtype)
    ple = ple_value(x, t, e)
    rank, pairs = rank_value(x, t, e, c.rank_gamma, c.rank_norm, fp32_weights)
    recon = recon_value(x, t, e, c.recon_alpha, c.recon_gamma, c.recon_norm)
    mse = mse_value(x, t, e, c.mse_censored)
    objective = x.sum() * 0.0
    for w, term in ((c.w_ple, ple), (c.w_rank, rank), (c.w_recon, recon), (c.w_mse, mse)):
        if w != 0:
            objective = objective + w * term
    (grad,) = torch.autograd.grad(objective, x)
    return Truth(ple.detach(), rank.detach(), recon.detach(), mse.detach(), pairs, objective.detach(), grad)


@functools.lru_cache(maxsize=None)
def case_truth(c, dtype=torch.float64, fp32_weights=False):
    i = case_inputs(c)
    return truth(i.pred, i.t, i.e, c, dtype, fp32_weights)


@functools.lru_cache(maxsize=None)
def edge_truth(name, l2=False, dtype=torch.float64):
    return truth(*EDGES[name], EDGE_CASE_L2 if l2 else EDGE_CASE, dtype)


def terms_with_weight(c):
    """{name of a Truth field: True where the launch computes it}: a term without a weight reads 0"""
    return dict(ple=c.w_ple != 0, rank=c.w_rank != 0, recon=c.w_recon != 0, mse=c.w_mse != 0)


def spec(c):
    """the keyword arguments of vlsa_amd.losses.SurvPairObjective for a case"""
    return dict(weight_ple=c.w_ple, weight_rank=c.w_rank, weight_recon=c.w_recon, weight_mse=c.w_mse, rank_gamma=c.rank_gamma,
                rank_norm=c.rank_norm, recon_alpha=c.recon_alpha, recon_gamma=c.recon_gamma, recon_norm=c.recon_norm,
                mse_include_censored=c.mse_censored)


# ---- a split: the Cox and Reg evaluators (vlsa_cox_risk_sets / vlsa_cox_cum_hazard / vlsa_cox_finish / vlsa_reg_eval, float64)
SPLIT_TILE = 256         # kSplitTile: samples per workgroup and per LDS tile
SPLIT_SHAPES = (2, 3, 65, 257, 1025)                  # the fixtures: tests/golden/cox_split_m<M>_<times>.npz
SPLIT_EDGES = (SPLIT_TILE - 1, SPLIT_TILE, SPLIT_TILE + 1, 2 * SPLIT_TILE + 1)      # against the restatement below
END_TIME = 12.0
REG_METRICS = ("loss", "loss_rank", "loss_recon", "loss_recon_org", "event_t_rae", "nonevent_t_rae", "event_t_nre", "nonevent_t_nre")
SplitInputs = collections.namedtuple("SplitInputs", "y_hat reg_pred t e")


@functools.lru_cache(maxsize=None)
def split_inputs(M, times):
    """y_hat [M] fp32 log-risks = randn * 2 (sample 2 on SurvPLE's cap, sample 3 above it from four samples on), reg_pred [M] fp32 predicted
    times = t + randn * 2, t [M] fp32 (no ties / integers 0 .. 11), e ~ Bernoulli(0.6); sample 0 is an event at the smallest time and,
    below four samples, sample 1 comes later: a comparable pair exists"""
    g = torch.Generator()
    g.manual_seed(7700 + 10 * M + TIMES.index(times))
    y_hat = torch.randn(M, generator=g) * 2.0
    if times == "ties":
        t = torch.randint(0, 12, (M,), generator=g).float()
        t[0] = 0.0
    else:
        t = (torch.randperm(M, generator=g).float() + 0.5 * torch.rand(M, generator=g)) * (12.0 / M)
        t[0] = t.min() * 0.5
    e = (torch.rand(M, generator=g) < 0.6).float()
    e[0] = 1.0
    if M < 4:
        t[1] = 5.0
    else:
        y_hat[2], y_hat[3] = CAP, 11.0
    reg_pred = t + torch.randn(M, generator=g) * 2.0
    return SplitInputs(y_hat, reg_pred, t, e)


def breslow(y_hat, t, e):
    """(sorted unique times [U], Breslow's cumulative baseline hazard there [U]) in float64 by the identity: H(u) = sum over the events
    with t_i <= u of 1 / D_i, D_i = sum_{j: t_j >= t_i} exp(y_hat_j), uncapped"""
    y, t, e = y_hat.double().reshape(-1), t.double().reshape(-1), e.double().reshape(-1)
    ex = torch.exp(y)
    D = ((t.view(1, -1) >= t.view(-1, 1)).double() * ex.view(1, -1)).sum(dim=1)
    times = torch.unique(t)
    inv = torch.where(e != 0, 1.0 / D, torch.zeros_like(D))
    H = ((t.view(1, -1) <= times.view(-1, 1)).double() * inv.view(1, -1)).sum(dim=1)
    return times, H


def breslow_by_subtraction(y_hat, t, e):
    """(times [U], H [U], a bound [U] on what H loses) the way the reference's BreslowEstimator forms it (eval/utils_coxph.py:215-232): the
    samples sorted by time, the risk-set sum of a time = the total minus the risk scores that left, one subtraction per unique time.
    That is not the identity's arithmetic: every subtraction rounds at the size of the TOTAL (2^-53 of it), and a late risk set is small,
    so its quotient carries up to u 2^-53 total / D_u of relative error after u steps.  `bound` adds that up along the cumulative sum."""
    y, tt, ee = y_hat.double().numpy().reshape(-1), t.double().numpy().reshape(-1), e.numpy().reshape(-1) != 0
    order = np.argsort(tt, kind="mergesort")
    risk, tt, ee = np.exp(y)[order], tt[order], ee[order]
    times, first = np.unique(tt, return_index=True)
    n_events = np.add.reduceat(ee.astype(np.int64), first)
    value, divisor = np.sum(risk), np.empty(len(times))
    divisor[0] = value
    for u in range(1, len(times)):
        value -= risk[first[u - 1]:first[u]].sum()
        divisor[u] = value
    H = np.cumsum(n_events / divisor)
    bound = np.cumsum(n_events / divisor ** 2 * (np.arange(len(times)) + 1) * 2.0 ** -53 * divisor[0])
    return torch.from_numpy(times), torch.from_numpy(H), torch.from_numpy(bound)


def survival_curves(y_hat, H):
    return torch.exp(-H.view(1, -1) * torch.exp(y_hat.double().reshape(-1, 1)))


def reg_metrics(pred, t, e, end_time=END_TIME, alpha=0.0, gamma=1.0, norm="l1", rank_gamma=1.0, rank_norm="l1"):
    """RegSurv_Evaluator's eight computable metrics (eval/evaluator_surv.py:424-458) in float64, and the number of rank pairs; loss_rank
    with the reference's fp32 pair weights, the number RegSurvEvaluator reproduces"""
    p, t, e = pred.double().reshape(-1), t.double().reshape(-1), e.double().reshape(-1)
    rank, pairs = rank_value(p, t, e, rank_gamma, rank_norm, fp32_weights=True)
    ev, ce = e == 1, e == 0
    out = {"loss": recon_value(p, t, e, 0.0, gamma, norm), "loss_rank": rank, "loss_recon": recon_value(p, t, e, alpha, gamma, norm),
           "loss_recon_org": recon_value(p, t, e, 0.0, gamma, norm),
           "event_t_rae": torch.mean(torch.abs(t[ev] - p[ev]) / end_time), "nonevent_t_rae": torch.mean(torch.relu(t[ce] - p[ce]) / end_time),
           "event_t_nre": torch.mean((p[ev] - t[ev]) / end_time), "nonevent_t_nre": torch.mean(-torch.relu(-(p[ce] - t[ce])) / end_time)}
    return {k: float(v) for k, v in out.items()}, pairs


def split_fixture_file(M, times):
    return f"cox_split_m{M}_{times}.npz"


def load_split_fixture(M, times):
    with np.load(os.path.join(GOLDEN, split_fixture_file(M, times)), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
