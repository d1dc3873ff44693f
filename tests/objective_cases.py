"""Cases and float64 truth of the handler's objectives beyond SurvIFMLE + SurvEMD (vlsa_amd/csrc/surv_objectives.hip): the hazard family --
SurvMLE and SurvEMD behind the sigmoid -- and SurvT2I, shared by tests/test_objective_cases_cpu.py (the restatement against the
reference's own float64 results in tests/golden/objective_*.npz, the input conditions, the gates) and tests/test_gpu_objectives.py (the
kernels).  CPU only: torch, tests/surv_eval_helpers.py and tests/surv_loss_cases.py (the incidence family's inputs)."""
import collections
import functools
import glob
import os

import numpy as np
import torch

import surv_eval_helpers as H
import surv_loss_cases as S

# ---- what the launches branch on (tests/test_objective_cases_cpu.py::test_dispatch_constants_match_the_source reads them from the code)
ROWS16_MAX_K = 16        # surv_objectives.hip, launch_terms: `if (a.K <= 16)` -> k_surv_terms_rows16, else k_surv_terms
CHUNK = 32               # kTermThreads = 32 (k_surv_terms), kTermWideSamples = kTermWide / 16 = 32 (rows16): samples per pass
T2I_GROUPS_ROWS16 = 32   # k_surv_terms_rows16: the SurvT2I column of bin k is walked by kTermWideSamples threads, thread g takes samples g, g + 32, ..
T2I_GROUPS_WIDE = 4      # k_surv_terms: kTermBlock / kTermCols = 256 / 64 threads per column
T2I_GROUPS_ALONE = 256   # k_t2i_columns (vlsa_surv_t2i): kT2iThreads threads per column; k_t2i_finish: as many elements per workgroup
ONE_BLOCK_MAX_B = 4096   # vlsa_surv_objective_terms: `B > kOneBlockMaxB` is refused; losses.py: ONE_LAUNCH_MAX_B
MAX_K = S.MAX_K
BATCH_EDGES = sorted({1, 130} | {g + d for g in (CHUNK, T2I_GROUPS_ROWS16, T2I_GROUPS_WIDE) for d in (-1, 0, 1)})

LOG_LOGIT_SCALE, LOGIT_SCALE, EPS = S.LOG_LOGIT_SCALE, S.LOGIT_SCALE, S.EPS
BAND = 1e-3              # a clamped quantity within a factor 1 +- BAND of eps: the side of the clamp hangs on the last ulp of ANY fp32 run
MAX_ALTERED = 0.25       # share of a case's samples an input rule may alter (the cap of surv_loss_cases.py)

# ---- the gates, per family: 8 x the worst error of a plain fp32 evaluation of the same formulas on the CPU (torch; 1 - h written as
# sigmoid(-x)) against the float64 truth, rounded up to one significant digit -- the method of surv_loss_cases.py.
# tests/test_objective_cases_cpu.py::test_gates_are_eight_times_the_fp32_restatement measures them on every case, the scale-12 table included,
# and asserts that the restatement stays within an eighth of each.  Measured worst cases:
#   hazard     value 1.44e-7 (relative to max(1, |value|): grid-hazard-k1-b33-CL); gradient 2.11e-7 (relative to max(largest float64 entry,
#              1 / B): grid-hazard-k2-b32-CL); at scale 12: 5.0e-8 and 1.34e-7
#   incidence  value 3.00e-7 (grid-incidence-k63-b1-CL); gradient 1.27e-5 (opt-incidence-k17-b33-KL-p2-a0-w1/1/0-mean: SurvIFMLE + SurvEMD,
#              the figure of surv_loss_cases.py); at scale 12: 9.1e-8 and 1.48e-6
#   per-sample route on given hazards (SurvMLE, SurvEMD; each sample relative to max(1, itself) / to its row's largest float64 entry):
#              values 1.60e-6 (SurvEMD, K = 15, B = 130), gradient rows 1.97e-5 (SurvEMD, K = 64, B = 31)
# The 1 / B floor is a definition: a B = 1 batch on a clamp has a float64 gradient of 1e-11, and fp32 owes nothing relative to that.
VALUE_RTOL = {"hazard": 2e-6, "incidence": 3e-6}
GRAD_RTOL = {"hazard": 2e-6, "incidence": 2e-4}
ROW_VALUE_RTOL = 2e-5
ROW_GRAD_RTOL = 2e-4
# SurvT2I alone (vlsa_surv_t2i) on the T2I_ALONE table -- up to 5000 samples in a softmax, and a logit scale of 2, where the KL targets of
# the non-positives do not vanish: value 1.16e-6, gradient 1.50e-6 (both K = 16, B = 5000, KL / mean at scale 2)
T2I_VALUE_RTOL = 1e-5
T2I_GRAD_RTOL = 2e-5

Case = collections.namedtuple("Case", "name family B K seed scale p raw alpha w_main w_emd w_t2i t2i_loss t2i_reduction all_events")
_DEFAULT_T2I = {"hazard": "CL", "incidence": "KL"}       # the pairing of the fixtures


def _case(prefix, family, B, K, scale, t2i_loss=None, t2i_reduction="mean", p=2, raw=True, alpha=0.0, w=(1.0, 1.0, 0.5), tag=""):
    t2i_loss = t2i_loss or _DEFAULT_T2I[family]
    seed = 5000 + 100 * K + B
    if family == "incidence":       # the seeds surv_loss_cases.py found for its own conditions at scale 12
        seed = S.SEEDS.get(("extreme" if scale == 12.0 else prefix, K, B), seed)
    return Case(f"{prefix}-{family}-k{K}-b{B}-{t2i_loss}{tag}", family, B, K, seed, scale, p, raw, alpha, w[0], w[1], w[2], t2i_loss, t2i_reduction,
                p == 2 and not raw)


FAMILIES = ("hazard", "incidence")
GRID = [_case("grid", f, B, K, 2.0, loss) for f in FAMILIES for K in (1, 2, 15, 16, 17, 63, 64) for B in BATCH_EDGES for loss in ("CL", "KL")]
EXTREME = [_case("extreme", f, 130, K, 12.0, loss) for f in FAMILIES for K in (16, 17, 64) for loss in ("CL", "KL")]
# 4097: the first batch SurvObjective sends down the per-sample launch + the SurvT2I launches + torch adds
BIG = [_case("big", f, B, K, 2.0) for f in FAMILIES for K in (16, 17) for B in (ONE_BLOCK_MAX_B - 1, ONE_BLOCK_MAX_B, ONE_BLOCK_MAX_B + 1)]
_DIST = {(2, True): "p2", (2, False): "p2root", (1, True): "p1"}
WEIGHTS = ((1.0, 1.0, 0.5), (0.0, 1.0, 0.5), (1.0, 0.0, 0.5), (1.0, 1.0, 0.0), (0.7, 1.3, 2.0))      # (likelihood term, SurvEMD, SurvT2I)
OPTIONS = [_case("opt", f, 33, K, 2.0, None, red, p, raw, alpha, w, f"-{_DIST[(p, raw)]}-a{alpha:g}-w{w[0]:g}/{w[1]:g}/{w[2]:g}-{red}")
           for f in FAMILIES for K in (12, 17) for (p, raw) in _DIST for alpha in (0.0, 0.3) for w in WEIGHTS for red in ("mean", "sum")]
OBJECTIVE_CASES = GRID + EXTREME + BIG + OPTIONS
# (K, B) of the grid whose draw holds no event: no SurvT2I bin is counted, the term and its gradient are zero
GRID_WITHOUT_COUNTED_BIN = {(2, 3), (15, 1), (17, 1), (63, 1)}
# the fixtures: the reference's own float64 results (tests/golden/make_golden_objectives.py)
FIXTURE_SHAPES = ((1, 4), (5, 12), (33, 16), (33, 17), (130, 64))
FIXTURES = [_case("fix", f, B, K, 2.0, None, red, alpha=alpha, tag=f"-a{alpha:g}-{red}")
            for f in FAMILIES for (B, K) in FIXTURE_SHAPES for alpha in (0.0, 0.3) for red in ("mean", "sum")]
# per-sample route on given hazards (vlsa_surv_terms, converter "none": the SurvMLE module, SurvEMD on hazards)
ROW_SHAPES = [(K, B) for K in (1, 15, 16, 17, 40, 64) for B in (1, 31, 32, 33, 130)]
ROW_LOGIT_SCALE = S.ROW_LOGIT_SCALE


# SurvT2I alone: (K, B, loss, reduction, logit scale); B around the threads that walk a column of vlsa_surv_t2i, and the evaluator's size
T2I_ALONE = [(K, B, loss, red, ls) for (K, B) in ((12, T2I_GROUPS_ALONE - 1), (17, T2I_GROUPS_ALONE), (64, T2I_GROUPS_ALONE + 1), (16, 5000))
             for (loss, red, ls) in (("CL", "mean", LOGIT_SCALE), ("KL", "sum", LOGIT_SCALE), ("KL", "mean", 2.0))]


def ids(cases):
    return [c.name for c in cases]


def fixture_file(c):
    """one file per family and shape: the inputs once, the results of its four (alpha, reduction) variants side by side"""
    return f"objective_{c.family}-k{c.K}-b{c.B}.npz"


def variant(c):
    return f"a{c.alpha:g}-{c.t2i_reduction}"


def load_fixture(c):
    """the fixture of ONE case: the shared entries, and the entries stored as `<variant>/<name>` under their name"""
    tag = variant(c) + "/"
    with np.load(os.path.join(H.GOLDEN, fixture_file(c)), allow_pickle=False) as z:
        out = {k: z[k] for k in z.files if "/" not in k}
        out.update({k[len(tag):]: z[k] for k in z.files if k.startswith(tag)})
    return out


def fixture_files():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(H.GOLDEN, "objective_*.npz")))


# ---- inputs
Inputs = collections.namedtuple("Inputs", "logits t e changed")


def clamped_quantities(logits, t, e):
    """[B, 2] float64: what SurvMLE clamps at eps for each sample -- (h_t, S_padded[t]) of an event, S_padded[t + 1] (twice) of a censored one"""
    x = logits.double()
    B, K = x.shape
    tc = t.clamp(0, K - 1).view(B, 1)
    sp = torch.cat([torch.ones(B, 1, dtype=torch.float64), torch.cumprod(torch.sigmoid(-x), dim=1)], 1)
    ev = torch.cat([torch.sigmoid(x).gather(1, tc), sp.gather(1, tc)], 1)
    return torch.where(e.view(B, 1) != 0, ev, sp.gather(1, tc + 1).expand(B, 2))


def in_band(logits, t, e):
    """[B] bool: a clamped quantity of the sample sits within a factor 1 +- BAND of eps"""
    return ((clamped_quantities(logits, t, e) / EPS - 1.0).abs() < BAND).any(dim=1)


@functools.lru_cache(maxsize=None)
def make_inputs(family, B, K, seed, scale, all_events=False):
    """logits [B, K] fp32 = randn * scale, t [B] int64 uniform in [0, K), e [B] fp32 ~ Bernoulli(0.45) -- the recipe of
    surv_loss_cases.make_inputs, whose tail rule is the incidence family's input rule (its inputs are taken as they are).  Hazard family:
    the logits of a sample in the band around the clamp (in_band) are drawn again.  `changed`: samples a rule altered.  (Cached: read-only.)"""
    if family == "incidence":
        return Inputs(*S.make_inputs(B, K, seed, scale, all_events))
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
    if all_events:
        e = torch.ones_like(e)
    altered = torch.zeros(B, dtype=torch.bool)
    for _ in range(100):
        band = in_band(logits, t, e)
        if not bool(band.any()):
            break
        altered |= band
        logits[band] = torch.randn(int(band.sum()), K, generator=g) * scale
    return Inputs(logits, t, e, int(altered.sum()))


def case_inputs(c):
    return make_inputs(c.family, c.B, c.K, c.seed, c.scale, c.all_events)


# ---- the float64 restatement
def mle_rows(h, one_minus_h, t, e, alpha=0.0, eps=EPS):
    """SurvMLE per sample [B] (loss/loss_surv.py:113-122 without the mean), 1 - h handed in: sigmoid(-x) behind the converter, 1 - h on
    given hazards.  t inside [0, K - 1]."""
    B = h.shape[0]
    t = t.view(B, 1)
    c = 1.0 - e.view(B, 1).to(h.dtype)
    sp = torch.cat([torch.ones_like(c), torch.cumprod(one_minus_h, dim=1)], 1)
    unc = -(1 - c) * (torch.log(sp.gather(1, t).clamp(min=eps)) + torch.log(h.gather(1, t).clamp(min=eps)))
    cen = -c * torch.log(sp.gather(1, t + 1).clamp(min=eps))
    return ((1.0 - alpha) * (cen + unc) + alpha * unc).view(B)


def t2i_bins(t, e, K):
    """(participates [B, K], positive [B, K]) of SurvT2I: the events and the censored samples with t > k; the events with t == k"""
    k = torch.arange(K).view(1, K)
    ev, tt = (e.view(-1, 1).long() != 0), t.view(-1, 1)
    return ev | (tt > k), ev & (tt == k)


def t2i_value(raw, t, e, logit_scale, loss="CL", reduction="mean"):
    """(SurvT2I of the raw logits, the number of counted bins): loss/loss_surv_ext.py:145-195 bin by bin, in raw's dtype; no counted
    bin: a zero of that dtype"""
    K = raw.shape[1]
    part, pos = t2i_bins(t, e, K)
    total, slots = torch.zeros((), dtype=raw.dtype), 0
    for i in range(K):
        sel = part[:, i]
        target = pos[:, i][sel].to(raw.dtype)
        if not bool(sel.any()) or float(target.sum()) == 0:
            continue
        lp = torch.log_softmax(raw[:, i][sel], dim=0)
        if loss == "CL":
            cur = -(target * lp).sum() / target.sum()
        else:
            td = torch.softmax((2 * target - 1) * logit_scale, dim=0)
            cur = (torch.xlogy(td, td) - td * lp).sum()
        total, slots = total + cur, slots + 1
    if reduction == "mean" and slots:
        total = total / slots
    return total, slots


Truth = collections.namedtuple("Truth", "main emd t2i slots objective grad")


def truth(x, t, e, logit_scale, family, alpha=0.0, eps=EPS, p=2, raw_distance=True, w_main=1.0, w_emd=1.0, w_t2i=0.0, t2i_loss="CL",
          t2i_reduction="mean", dtype=torch.float64):
    """per-sample likelihood term [B] (SurvMLE of sigmoid(x) / SurvIFMLE of softmax(x)) and SurvEMD [B], SurvT2I, objective =
    mean_i (w_main main_i + w_emd emd_i) + w_t2i T2I and d objective / d x [B, K] by autograd, all in `dtype` (float64: the truth;
    float32: the plain fp32 restatement the gates are measured on).  t is clamped into [0, K - 1] as the kernels clamp it."""
    x = x.detach().to(dtype).requires_grad_(True)
    t = t.clamp(0, x.shape[1] - 1)
    if family == "hazard":
        y = torch.sigmoid(x)
        main = mle_rows(y, torch.sigmoid(-x), t, e, alpha, eps)
    else:
        y = torch.softmax(x, dim=-1)
        main = H.loss_mle(y, t, e, "incidence", alpha, eps, reduce=False, dtype=dtype)
    emd = H.loss_emd_rows(y, t, e, logit_scale, p, raw_distance, dtype=dtype)
    t2i, slots = t2i_value(x, t, e, logit_scale, t2i_loss, t2i_reduction)
    objective = (w_main * main + w_emd * emd).mean() + w_t2i * t2i
    (grad,) = torch.autograd.grad(objective, x)
    return Truth(main.detach(), emd.detach(), t2i.detach(), slots, objective.detach(), grad)


@functools.lru_cache(maxsize=None)
def case_truth(c, dtype=torch.float64):
    i = case_inputs(c)
    return truth(i.logits, i.t, i.e, LOGIT_SCALE, c.family, c.alpha, EPS, c.p, c.raw, c.w_main, c.w_emd, c.w_t2i, c.t2i_loss, c.t2i_reduction, dtype)


@functools.lru_cache(maxsize=None)
def row_inputs(K, B):
    """(hazards [B, K] fp32, t, e) of the per-sample route"""
    i = make_inputs("hazard", B, K, 7000 + 100 * K + B, 2.0)
    return torch.sigmoid(i.logits), i.t, i.e


@functools.lru_cache(maxsize=None)
def row_truth(K, B, which, dtype=torch.float64):
    """per-sample values [B] and gradient rows [B, K] (d loss_i / d hazard_i) of SurvMLE or SurvEMD on row_inputs"""
    h, t, e = row_inputs(K, B)
    h = h.to(dtype).requires_grad_(True)
    rows = mle_rows(h, 1 - h, t, e) if which == "mle" else H.loss_emd_rows(h, t, e, ROW_LOGIT_SCALE, 2, True, dtype=dtype)
    (grad,) = torch.autograd.grad(rows.sum(), h)
    return rows.detach(), grad


@functools.lru_cache(maxsize=None)
def t2i_alone_truth(K, B, loss, reduction, ls, dtype=torch.float64):
    i = make_inputs("hazard", B, K, 8000 + 100 * K + B, 2.0)
    return truth(i.logits, i.t, i.e, ls, "hazard", w_main=0.0, w_emd=0.0, w_t2i=1.0, t2i_loss=loss, t2i_reduction=reduction, dtype=dtype)


# ---- edges, each its own small case: name -> (logits [B, K] fp32, t, e) for a bin count K >= 4
def _edge(rows, K, seed):
    """rows: (t, e, {bin: logit}) per sample; the other logits are randn"""
    g = torch.Generator()
    g.manual_seed(seed)
    logits = torch.randn(len(rows), K, generator=g)
    for b, (_, _, fixed) in enumerate(rows):
        for k, v in fixed.items():
            logits[b, k] = v
    return logits, torch.tensor([r[0] for r in rows], dtype=torch.int64), torch.tensor([float(r[1]) for r in rows])


EDGES = {
    "event-at-t0": lambda K: _edge([(0, 1, {}), (2, 0, {}), (1, 1, {})], K, 1),
    "censored-in-the-last-bin": lambda K: _edge([(K - 1, 0, {}), (1, 1, {}), (K - 1, 1, {})], K, 2),
    # h_t = sigmoid(-20) = 2e-9 < eps: the clamped value, and no gradient through that clamp
    "h-below-eps": lambda K: _edge([(2, 1, {2: -20.0}), (1, 1, {}), (3, 0, {})], K, 3),
    # S_padded[t] and S_padded[t + 1] <= sigmoid(-20) < eps for the event and the censored sample behind bin 0
    "survival-below-eps": lambda K: _edge([(2, 1, {0: 20.0}), (3, 0, {0: 20.0}), (0, 1, {})], K, 4),
    "t-outside-the-bins": lambda K: _edge([(-3, 1, {}), (K + 5, 1, {}), (K, 0, {}), (-1, 0, {}), (1, 1, {})], K, 5),
    "all-censored": lambda K: _edge([(1, 0, {}), (K - 3, 0, {}), (2, 0, {})], K, 6),                     # no counted bin
    "one-event": lambda K: _edge([(1, 1, {})], K, 7),                                                    # log-softmax of one entry: 0
    "censored-at-t0": lambda K: _edge([(0, 0, {}), (1, 1, {}), (2, 1, {})], K, 8),                       # takes part in no bin
    # bin 0 has participants (every event, the censored sample with t = 2) and no positive; bin 1 is counted
    "bin-without-a-positive": lambda K: _edge([(1, 1, {}), (2, 0, {}), (1, 1, {}), (3, 1, {})], K, 9),
}
NO_COUNTED_BIN = ("all-censored",)
# The incidence family leaves out the two edges named for SurvMLE's clamps and the two that put a censored sample into the last bin:
# SurvIFMLE takes log(clamp(1 - CIF, eps)) of a difference that is rounding noise there, decided by the last ulp of any fp32 run
# (tests/test_gpu_losses.py keeps that edge's own test)
_HAZARD_ONLY = ("h-below-eps", "survival-below-eps", "censored-in-the-last-bin", "t-outside-the-bins")
EDGE_NAMES = {"hazard": tuple(EDGES), "incidence": tuple(n for n in EDGES if n not in _HAZARD_ONLY)}
EDGE_BINS = (5, 17)      # one bin count per kernel


@functools.lru_cache(maxsize=None)
def edge_truth(name, K, family, t2i_loss, dtype=torch.float64):
    x, t, e = EDGES[name](K)
    return truth(x, t, e, LOGIT_SCALE, family, 0.3, EPS, 2, True, 1.0, 1.0, 0.5, t2i_loss, "mean", dtype)


# ---- error measures
def rel_value(got, want):
    """|got - want| / max(1, |want|)"""
    got, want = float(got), float(want)
    return abs(got - want) / max(1.0, abs(want))


def rel_grad(got, want, B=None):
    """max|got - want| relative to max(the largest entry of the float64 gradient, 1 / B)"""
    got, want = got.double(), want.double()
    B = want.shape[0] if B is None else B
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1.0 / B)


rel_value_rows = S.rel_value_rows
