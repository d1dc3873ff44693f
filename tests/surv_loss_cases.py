"""Cases and float64 truth of the survival loss kernels on the incidence family (vlsa_amd/csrc/surv_objectives.hip: k_surv_terms_rows16 up
to 16 bins, k_surv_terms for 17 .. 64), shared by tests/test_surv_loss_cases_cpu.py (the input conditions, the gates) and tests/test_gpu_surv_loss_edges.py (the
kernels).  CPU only: torch and tests/surv_eval_helpers.py, whose loss formulas tests/test_surv_eval_cpu.py pins to the reference's
float64 results."""
import collections
import functools
import math

import torch

import surv_eval_helpers as H

# ---- what the launches branch on
ROWS16_MAX_K = 16        # surv_objectives.hip, launch_terms: `if (a.K <= 16)` -> k_surv_terms_rows16, else k_surv_terms
CHUNK = 32               # surv_objectives.hip: kTermThreads = 32 (k_surv_terms), kTermWideSamples = kTermWide / 16 = 32 (rows16) samples per pass
ONE_BLOCK_MAX_B = 4096   # surv_objectives.hip: kOneBlockMaxB, a larger B is refused; losses.py: ONE_LAUNCH_MAX_B
MAX_K = 64               # include/vlsa_hip.h: VLSA_MAX_K

LOG_LOGIT_SCALE = 4.0309                        # the shipped checkpoint's parameter (tests/golden/cases.py LOGIT_SCALE)
LOGIT_SCALE = math.exp(LOG_LOGIT_SCALE)         # 56.3
MIN_TAIL = 1e-2                                 # a censored sample keeps at least this much mass behind its bin (see make_inputs)
EPS = 1e-7

# ---- the gates: 8 x the worst error of a plain fp32 evaluation of the same formulas on the CPU (torch; the kernels may order their sums
# and take expf / logf differently: another constant in front of the rounding error, not another order of magnitude), rounded up to one
# significant digit.  tests/test_surv_loss_cases_cpu.py::test_gates_are_eight_times_the_fp32_restatement measures them on every case and
# asserts that the restatement stays within an eighth of each.  Measured worst cases:
#   VALUE_RTOL      3.0e-7  the objective, relative to itself (grid-k63-b1)
#   GRAD_RTOL       1.27e-5 the objective's gradient, relative to its largest float64 entry (opt-k17-b33-p2-a0-w0.7/0);
#                   2.30e-5 the per-sample route's gradient rows, each relative to its own largest float64 entry (SurvEMD, K = 64, B = 31)
#   ROW_VALUE_RTOL  1.68e-6 the per-sample route's values, each relative to max(1, itself) (SurvEMD, K = 15, B = 31: see rel_value_rows)
VALUE_RTOL = 3e-6
GRAD_RTOL = 2e-4
ROW_VALUE_RTOL = 2e-5

Case = collections.namedtuple("Case", "name B K seed scale p raw alpha w_ifmle w_emd all_events")


def _case(prefix, B, K, scale, p=2, raw=True, alpha=0.0, w=(1.0, 1.0), tag=""):
    return Case(f"{prefix}-k{K}-b{B}{tag}", B, K, SEEDS.get((prefix, K, B), 5000 + 100 * K + B), scale, p, raw, alpha, w[0], w[1],
                p == 2 and not raw)


# (table, K, B) -> seed where 5000 + 100 K + B misses a condition of tests/test_surv_loss_cases_cpu.py::_check_inputs.  At scale 12 the
# softmax is nearly one-hot: the first seeds of the form 5130 + 100 K + 10000 j whose draw turns at most 25 % of the samples into events
# and puts no event's inc[t] into the band around eps
SEEDS = {("extreme", 16, 130): 1026730, ("extreme", 17, 130): 86830, ("extreme", 64, 130): 371530}

GRID = [_case("grid", B, K, 2.0) for K in (1, 2, 15, 16, 17, 31, 32, 33, 63, 64) for B in (1, 31, 32, 33, 130)]
# 4097: the first batch SurvObjective sends down the per-sample route + torch mean
BIG = [_case("big", B, K, 2.0) for K in (16, 17) for B in (ONE_BLOCK_MAX_B - 1, ONE_BLOCK_MAX_B, ONE_BLOCK_MAX_B + 1)]
EXTREME = [_case("extreme", 130, K, 12.0) for K in (16, 17, 64)]
_DIST = {(2, True): "p2", (2, False): "p2root", (1, True): "p1"}
OPTIONS = [_case("opt", 33, K, 2.0, p, raw, alpha, w, f"-{_DIST[(p, raw)]}-a{alpha:g}-w{w[0]:g}/{w[1]:g}")
           for K in (12, 16, 17, 40) for (p, raw) in _DIST for alpha in (0.0, 0.3) for w in ((1.0, 1.0), (0.7, 0.0), (0.0, 1.3), (0.5, 2.0))]
OBJECTIVE_CASES = GRID + BIG + EXTREME + OPTIONS

# the per-sample route (vlsa_surv_loss on incidences, SurvIFMLE / SurvEMD with reduction = 'none')
ROW_SHAPES = [(K, B) for K in (1, 15, 16, 17, 40, 64) for B in (1, 31, 32, 33, 130)]
# SurvEMD's logit scale there.  At the trained scale (56.3) a censored sample's gradient row is e^-56 times the difference of two cdfs
# that agree to rounding: 1e-48 in float64 and noise in ANY fp32 evaluation, so "relative to the row's own largest entry" has no fp32
# answer.  At 2.0 every row -- censored ones too -- is well conditioned, and the kernel runs the same instructions.
ROW_LOGIT_SCALE = 2.0


def ids(cases):
    return [c.name for c in cases]


Inputs = collections.namedtuple("Inputs", "logits t e changed")


@functools.lru_cache(maxsize=None)
def make_inputs(B, K, seed, scale, all_events=False):
    """logits [B, K] fp32 = randn * scale, t [B] int64 uniform in [0, K), e [B] fp32 ~ Bernoulli(0.45); `changed`: how many censored
    samples the tail rule turned into events.  (Cached: treat the tensors as read-only.)"""
    g = torch.Generator()
    g.manual_seed(seed)
    logits = torch.randn(B, K, generator=g) * scale
    t = torch.randint(0, K, (B,), generator=g)
    e = (torch.rand(B, generator=g) < 0.45).float()
    if B >= 4:      # the four samples tests/test_gpu_losses.py::_inputs forces
        t[0], e[0] = 0, 1.0
        t[1], e[1] = max(K - 2, 0), 0.0
        t[2], e[2] = K - 1, 1.0
        t[3], e[3] = 0, 0.0
    changed = 0
    if K > 1:
        # a censored sample contributes -log(1 - CIF[t]) and the gradient c / (1 - CIF[t]): below MIN_TAIL of remaining mass the rounding of
        # an fp32 cumulative sum (6e-8 per add) is magnified past any useful gate, and at the clamp itself (a censored sample in the last
        # bin) the reference's own result hangs on the last ulp -- tests/test_gpu_losses.py keeps that edge's dedicated test.
        # (K = 1: 1 - 1 is exactly 0 in any precision, the clamp is exact: censored samples stay.)
        tail = 1.0 - torch.cumsum(torch.softmax(logits.double(), dim=-1), dim=-1).gather(1, t.view(-1, 1)).view(-1)
        flip = (e == 0) & (tail < MIN_TAIL)
        changed = int(flip.sum())
        e = torch.where(flip, torch.ones_like(e), e)
    if all_events:
        e = torch.ones_like(e)
    return Inputs(logits, t, e, changed)


def case_inputs(c):
    return make_inputs(c.B, c.K, c.seed, c.scale, c.all_events)


Truth = collections.namedtuple("Truth", "ifmle emd objective grad")


def truth(x, t, e, logit_scale, alpha=0.0, eps=EPS, p=2, raw_distance=True, w_ifmle=1.0, w_emd=1.0, from_logits=True, dtype=torch.float64):
    """per-sample SurvIFMLE [B] and SurvEMD [B], objective = mean_i (w_ifmle ifmle_i + w_emd emd_i) and d objective / d x [B, K] by
    autograd, all evaluated in `dtype` (float64: the truth; float32: the plain fp32 restatement the gates are measured on)"""
    x = x.detach().to(dtype).requires_grad_(True)
    inc = torch.softmax(x, dim=-1) if from_logits else x
    ifmle = H.loss_mle(inc, t, e, "incidence", alpha, eps, reduce=False, dtype=dtype)
    emd = H.loss_emd_rows(inc, t, e, logit_scale, p, raw_distance, dtype=dtype)
    objective = (w_ifmle * ifmle + w_emd * emd).mean()
    (grad,) = torch.autograd.grad(objective, x)
    return Truth(ifmle.detach(), emd.detach(), objective.detach(), grad)


@functools.lru_cache(maxsize=None)
def case_truth(c, dtype=torch.float64):
    i = case_inputs(c)
    return truth(i.logits, i.t, i.e, LOGIT_SCALE, c.alpha, EPS, c.p, c.raw, c.w_ifmle, c.w_emd, True, dtype)


@functools.lru_cache(maxsize=None)
def row_inputs(K, B):
    """(incidences [B, K] fp32, t, e) of the per-sample route"""
    i = make_inputs(B, K, 7000 + 100 * K + B, 2.0)
    return torch.softmax(i.logits, dim=-1), i.t, i.e


@functools.lru_cache(maxsize=None)
def row_truth(K, B, which, dtype=torch.float64):
    """per-sample values [B] and per-sample gradient rows [B, K] (d loss_i / d incidence_i) of SurvIFMLE or SurvEMD on row_inputs"""
    inc, t, e = row_inputs(K, B)
    w = (1.0, 0.0) if which == "ifmle" else (0.0, 1.0)
    r = truth(inc, t, e, ROW_LOGIT_SCALE, 0.0, EPS, 2, True, w[0], w[1], False, dtype)
    return (r.ifmle if which == "ifmle" else r.emd), r.grad * B          # (the mean's 1 / B taken out again: exact for a power of two, 1 ulp else)


# ---- error measures
def rel_value(got, want):
    """|got - want| / |want| (a float64 tensor or a float each); a zero truth (K = 1 without censored samples) admits zero only"""
    got, want = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    err, ref = (got - want).abs(), want.abs()
    return float(torch.where(ref > 0, err / ref.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), err)).max())


def rel_value_rows(got, want):
    """per-sample values: max_i |got_i - want_i| / max(1, |want_i|).  Both losses are functions of probabilities in [0, 1] --
    -log(x), sums of squared cdf differences -- so one fp32 rounding of x = 1 - 1e-4 (6e-8) is an absolute error of 6e-8 in a loss of
    1e-4: a sample's loss is resolved to VALUE_RTOL of the larger of itself and 1, not of itself."""
    got, want = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    return float(((got - want).abs() / want.abs().clamp(min=1.0)).max())


def rel_grad(got, want):
    """max|got - want| relative to the LARGEST entry of the float64 gradient (no max(1, .)); an all-zero truth (K = 1: the softmax of
    one logit is constant) admits zeros only"""
    got, want = got.double(), want.double()
    err, ref = float((got - want).abs().max()), float(want.abs().max())
    return err / ref if ref > 0 else (0.0 if err == 0 else math.inf)


def rel_grad_rows(got, want):
    """rel_grad row by row: each sample's gradient against that row's own largest float64 entry; the worst row"""
    return max(rel_grad(got[i], want[i]) for i in range(want.shape[0]))
