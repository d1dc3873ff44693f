"""Cases, input recipes and float64 references for the head and tail kernels of vlsa_amd/csrc/vlfan_tail.hip and the merge-and-pool
kernels of vlsa_amd/csrc/vlfan_batch.hip: partial merge, query pooling, visual adapter, both normalisations, cosine logits, incidence,
the head's backward and the query chain rule.  Plain torch-CPU: nothing here touches a GPU or the native library.

The tail chooses among about ten kernels at run time from D, B, G, K, the pooling mode, the adapter and pointer alignment.
``expected_path`` restates those choices (and the host refusals); ``CASES`` names at least one case per reachable combination at the
smallest values where each branch flips; ``make_inputs`` / ``reference`` / ``fp32_eval`` are the recipes, the float64 reference and
torch's own fp32 evaluation of the same formulas (the evidence that a correct fp32 kernel can meet the gates).

Entries (``Case.entry``):
  head_forward       VF.head_forward -> vlsa_head_forward: the ticketed k_head, one bag
  head_batch         vlsa_head_forward_batch: k_pool_rows + k_head_linear(_mfma) + k_head_finish, or the ticketed grid (NB, B)
  head_batch_text    vlsa_head_forward_batch_text: the same with the K text rows normalised by K more workgroups of k_pool_rows
  merge_head         vlsa_vlfan_merge_head: k_vlfan_merge_wpart + k_head_finish_parts (fused) or k_vlfan_merge + k_head
  merge_head_batch   vlsa_vlfan_merge_head_batch_strided: k_vlfan_merge_pool_small (G <= 8) / _batch + the pooled route
  head_backward      vlsa_head_backward_batch: k_head_bwd_dv + k_head_bwd_params
  head_train         VF.head_train: the forward (batch_text, or normalize_rows + ticketed B = 1) and the backward as one autograd node
  query_chain        vlsa_query_chain: k_query_chain

Not a case on purpose: a W or ``pooled`` pointer that is not 16-byte aligned.  k_head, k_head_linear and the pooling store of
k_vlfan_merge_pool_batch move float4 through them with no host check: alignment is a precondition of the ABI (include/vlsa_hip.h,
DESIGN.md), torch's allocator gives 256 bytes.  The predicate ``pointers aligned`` of the MFMA adapter and of the fused single-slide
tail is therefore always true under test; their misaligned branch (k_head_linear / the unfused route) is the same kernel the other
widths run.

An empty partial record is (max -inf, sum 0, accumulator 0): what a streaming workgroup that got no rows writes (vlfan_batch.hip, the
group epilogue: M = -inf, lsum = 0, acc = 0 -> pm = -inf, pl = 0 * 0 + 0 * 0, pacc = 0) and what VF.vlfan_partial fills in for N = 0.
"""
import math
import zlib
from dataclasses import dataclass

import torch
import torch.nn.functional as TF

MAX_D, MAX_P, MAX_K, P_STRIDE = 1024, 16, 64, 16      # VLSA_MAX_D / _P / _K, kPStride
LOGIT_SCALE = 4.0309                                   # cases.LOGIT_SCALE, the shipped checkpoint's value
LS_100 = math.log(100.0)
NORM_EPS = 1e-12                                       # kNormEps: F.normalize's clamp, forward and backward
POOL_CODE = {"mean": 0, "max": 1, "weight": 2, "given": 3}
ENTRIES = ("head_forward", "head_batch", "head_batch_text", "merge_head", "merge_head_batch", "head_backward", "head_train",
           "query_chain")

# ---- gates: what the suite already asserts for these kernels ------------------------------------------------------------------------
GATE_LOGITS = 1e-4        # absolute                test_gpu_tails.py
GATE_VHAT = 1e-5          # absolute                test_gpu_tails.py
GATE_THAT = 1e-5          # absolute                by analogy with vhat (no existing gate)
GATE_INCIDENCE = 1e-4     # absolute                test_gpu_tails.py
GATE_ROWS = 1e-4          # x max(1, max|ref|)      test_gpu_tails.py: merged rows, pooled (and v, vnorm, tnorm, m2, l: the same kind)
GATE_GRAD = 1e-4          # of the reference tensor's largest entry: BASELINE.md section 3
_ABS = {"logits": GATE_LOGITS, "vhat": GATE_VHAT, "That": GATE_THAT, "incidence": GATE_INCIDENCE}
_GRADS = ("drows", "dW", "db", "dT", "dls", "dQ")

# The gates are held as they stand on every recipe: torch's fp32 CPU evaluation of every case leaves more than 2x room below each of them
# (tests/test_head_path_cases_cpu.py measures it and asserts it; worst 0.15 of the logits gate on near-parallel rows with 17 bags, 0.10
# on randn at D = 12, 0.07 at ls = log 100, 0.10 on d logit_scale, every other gradient below 0.01), so no recipe needs a wider one.


@dataclass(frozen=True)
class Case:
    entry: str
    B: int = 1
    P: int = 1
    D: int = 512
    K: int = 4
    G: int = 0                    # partial records (merge entries)
    mode: str = "mean"            # mean / max / weight / given
    adapter: bool = True          # W present
    bias: bool = True             # b present (only with an adapter)
    inc: bool = True              # incidence wanted
    recipe: str = "randn"
    layout: str = "contig"        # merge_head_batch: "strided" = spare floats between records and between bags;  head_batch: "inplace" = pooled == rows
    gv: bool = False              # head_backward: g_vhat given
    gt: bool = False              # head_backward: g_That given
    nq: int = 0                   # query_chain
    gated: bool = False
    ls: float = LOGIT_SCALE

    @property
    def id(self):
        s = f"{self.entry}-B{self.B}-P{self.P}-D{self.D}-K{self.K}"
        if self.G:
            s += f"-G{self.G}"
        if self.entry == "query_chain":
            return f"query_chain-nq{self.nq}-{'gated' if self.gated else 'plain'}-D{self.D}-{self.recipe}"
        s += f"-{self.mode}-A{int(self.adapter)}"
        s += "" if self.bias or not self.adapter else "-nob"
        s += "" if self.inc else "-noinc"
        s += "" if self.layout == "contig" else f"-{self.layout}"
        s += ("-gv" if self.gv else "") + ("-gt" if self.gt else "")
        s += "" if self.ls == LOGIT_SCALE else f"-ls{self.ls:.3g}"
        return s + f"-{self.recipe}"


# ---- the dispatch, restated ----------------------------------------------------------------------------------------------------------
def head_nb(D, adapter):
    """workgroups of the ticketed k_head per bag: 8 rows of W each, one without an adapter"""
    return (D + 7) // 8 if adapter else 1


def _pooled_route(B, D, K, adapter):
    """vlsa_launch_head_pooled_batch: adapter kernel + score path of k_head_finish"""
    lin = "copy" if not adapter else ("mfma" if D == 512 and B >= 16 else "valu")
    return (lin, "pre" if D <= 512 and K <= 16 else "inplace")


def _nb_kind(D, adapter):
    return "nb1" if not adapter else ("nb_half" if D % 8 == 4 else "nb_full")


def expected_path(entry, B=1, P=1, D=512, K=4, G=0, mode="mean", adapter=True, layout="contig", pool_w=True, nq=0, gated=False,
                  strides_ok=True):
    """The kernels an entry point launches, as a tuple of labels -- or the refusal "einval"."""
    fwd_bad = D <= 0 or D > MAX_D or D % 4 or not 1 <= P <= MAX_P or not 1 <= K <= MAX_K or B < 1 or (mode == "weight" and not pool_w)
    if entry == "head_forward":
        return "einval" if fwd_bad else ("ticketed", _nb_kind(D, adapter))
    if entry == "head_batch":
        if fwd_bad:
            return "einval"
        if B > 1 and mode != "given" and layout != "inplace":
            return ("rows",) + _pooled_route(B, D, K, adapter)
        return ("ticketed", _nb_kind(D, adapter), "grid_b" if B > 1 else "one_bag")
    if entry == "head_batch_text":
        if fwd_bad or mode == "given" or layout == "inplace":
            return "einval"
        return ("rows",) + _pooled_route(B, D, K, adapter)
    if entry == "merge_head":
        if fwd_bad or D % 8 or G < 1:
            return "einval"
        rounds = "one_round" if G <= 256 else "two_rounds"
        if D == 512 and adapter and mode in ("mean", "weight"):
            return ("fused", rounds)
        return ("unfused", _nb_kind(D, adapter))
    if entry == "merge_head_batch":
        if fwd_bad or mode == "given" or G < 1 or not strides_ok:
            return "einval"
        return ("small" if G <= 8 else "batch",) + _pooled_route(B, D, K, adapter)
    if entry == "head_backward":
        if D < 1 or D > MAX_D or not 1 <= P <= MAX_P or not 1 <= K <= MAX_K or B < 1:
            return "einval"
        return ("dw_chunks_1" if B <= 64 else "dw_chunks_many") if adapter else "identity", \
               ("bags8_full" if B % 8 == 0 else "bags8_ragged"), ("cols32_full" if D % 32 == 0 else "cols32_ragged")
    if entry == "head_train":
        if B > 1:
            return ("batch_text",) + _pooled_route(B, D, K, adapter)
        return ("ticketed", _nb_kind(D, adapter), "one_bag")
    if entry == "query_chain":
        Pq = nq - 1 if gated else nq
        if nq < 1 or nq > MAX_P + 1 or Pq < 1 or D < 1 or D > MAX_D:
            return "einval"
        return ("gated" if gated else "plain",)
    raise ValueError(entry)


def backward_counts(B, D, adapter):
    """(chunks of 64 bags the dW blocks walk, d-pooled workgroups, rounds of 16 bags of the dT / dls loops, j per thread slice)"""
    return ((B + 63) // 64 if adapter else 0, ((D + 31) // 32) * ((B + 7) // 8), (B + 15) // 16, (D + 7) // 8)


def case_path(c):
    return expected_path(c.entry, B=c.B, P=c.P, D=c.D, K=c.K, G=c.G, mode=c.mode, adapter=c.adapter, layout=c.layout, nq=c.nq,
                         gated=c.gated)


# every (entry, path) the library can reach: the coverage table of the CPU test has no empty row among these
def required_paths():
    nb = ("nb1", "nb_half", "nb_full")
    pooled = [(lin, fin) for lin in ("copy", "valu") for fin in ("pre", "inplace")] + [("mfma", "pre"), ("mfma", "inplace")]
    req = [("head_forward", ("ticketed", k)) for k in nb]
    req += [("head_batch", ("rows",) + r) for r in pooled]
    req += [("head_batch", ("ticketed", k, g)) for k in nb for g in ("grid_b", "one_bag")]
    req += [("head_batch_text", ("rows",) + r) for r in pooled]
    req += [("merge_head", ("fused", r)) for r in ("one_round", "two_rounds")] + [("merge_head", ("unfused", k)) for k in ("nb1", "nb_full")]
    # (merge_head refuses D % 8 != 0, so its unfused route never runs a half-empty last workgroup: unreachable, no case)
    req += [("merge_head_batch", (m,) + r) for m in ("small", "batch") for r in pooled]
    req += [("head_backward", (a, b8, c32)) for a in ("identity", "dw_chunks_1", "dw_chunks_many") for b8 in ("bags8_full", "bags8_ragged")
            for c32 in ("cols32_full", "cols32_ragged")]
    req += [("head_train", ("batch_text", "copy", "pre")), ("head_train", ("batch_text", "valu", "inplace")),
            ("head_train", ("ticketed", "nb1", "one_bag")), ("head_train", ("ticketed", "nb_full", "one_bag"))]
    req += [("query_chain", ("gated",)), ("query_chain", ("plain",))]
    return req


# ---- the case list ------------------------------------------------------------------------------------------------------------------
WIDTHS = (4, 12, 252, 256, 508, 512, 516, 768, 1020, 1024)
BAGS = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
QUERIES = (1, 2, 12, 16)
RANKS = (1, 4, 16, 17, 63, 64)
G_SINGLE = (1, 15, 16, 17, 255, 256, 257, 512)
G_BATCH = (1, 2, 7, 8, 9, 10, 16, 17, 33)
MODES = ("mean", "max", "weight")
FWD_RECIPES = ("parallel", "norm1e3", "norm1e-6", "zero_pooled", "max_ties", "sat_weight")
MERGE_RECIPES = ("empty_first", "empty_middle", "empty_last", "spread60")
BWD_RECIPES = ("parallel", "norm1e3", "norm1e-6", "zero_pooled", "dl_onehot", "dl_zero")


def _rot(seq, i):
    return seq[i % len(seq)]


def _recipe_fields(recipe, base):
    """the fields a recipe forces: zero_pooled needs the identity adapter, max_ties max pooling over >= 2 rows, sat_weight weight pooling"""
    f = dict(base, recipe=recipe)
    if recipe == "zero_pooled":
        f.update(adapter=False)
        if f.get("mode") == "max" or f.get("mode") == "given":
            f.update(mode="mean")
    elif recipe == "max_ties":
        f.update(mode="max", P=max(2, f.get("P", 1)))
    elif recipe == "sat_weight":
        f.update(mode="weight", P=max(2, f.get("P", 1)))
    return f


def _build_cases():
    cs = []
    add = lambda entry, **kw: cs.append(Case(entry, **kw))  # noqa: E731
    # -- vlsa_head_forward: every width with and without the adapter; P, K, the mode rotate (given with P = 1)
    for i, D in enumerate(WIDTHS):
        for a in (True, False):
            mode = _rot(MODES + ("given",), i + a)
            add("head_forward", P=1 if mode == "given" else _rot(QUERIES, i + a), D=D, K=_rot(RANKS, i), mode=mode, adapter=a,
                bias=not (a and i % 3 == 0), inc=(i + a) % 4 != 0)
    for D in (252, 512, 1024):
        for r in FWD_RECIPES:
            add("head_forward", **_recipe_fields(r, dict(P=12, D=D, K=4)))
        add("head_forward", P=12, D=D, K=4, ls=0.0)
        add("head_forward", P=12, D=D, K=17, ls=LS_100, recipe="ls100")
    # -- vlsa_head_forward_batch, rows route: every B at D = 512 (VALU below 16 bags, MFMA from 16 with its ragged tiles) and at another
    #    width (VALU with >= 16 bags, ragged groups of 8); K 16 / 17 flips `pre`; then the identity adapter (copy)
    for i, B in enumerate(BAGS[1:]):
        for D in (512, _rot(tuple(w for w in WIDTHS if w != 512), i)):
            add("head_batch", B=B, P=_rot(QUERIES, i), D=D, K=_rot(RANKS, i + (D == 512)), mode=_rot(MODES, i), bias=i % 4 != 1,
                inc=i % 3 != 2)
    for D in (252, 508, 512, 516):
        for K in (16, 17):
            for B in (9, 17):
                add("head_batch", B=B, P=2, D=D, K=K, mode="max")
            add("head_batch", B=9, P=12, D=D, K=K, mode="weight", adapter=False)
    #    ticketed route: one bag; B > 1 under given pooling and under pooled == rows -- the grid (NB, B)
    for i, D in enumerate(WIDTHS):
        add("head_batch", B=1, P=_rot(QUERIES, i), D=D, K=_rot(RANKS, i), mode=_rot(MODES, i), adapter=i % 3 != 0)
        add("head_batch", B=_rot((2, 5, 9, 17), i), P=1, D=D, K=_rot(RANKS, i + 1), mode="given", adapter=i % 2 == 1)
        add("head_batch", B=_rot((5, 2, 17, 9), i), P=1, D=D, K=_rot(RANKS, i + 2), mode="given", adapter=i % 2 == 0, layout="inplace")
    #    ... and under mean / max / weight with pooled == rows (P = 1: the rows are the pooled vectors, k_head does not store them again)
    for i, mode in enumerate(MODES):
        for D, a in ((512, True), (508, True), (768, False)):
            add("head_batch", B=_rot((3, 9, 17), i), P=1, D=D, K=_rot(RANKS, i + 1), mode=mode, adapter=a, layout="inplace")
    for D, B in ((516, 9), (512, 17)):
        for r in FWD_RECIPES:
            add("head_batch", **_recipe_fields(r, dict(B=B, P=12, D=D, K=4)))
        add("head_batch", B=B, P=12, D=D, K=4, ls=0.0)
        add("head_batch", B=B, P=12, D=D, K=17, ls=LS_100, recipe="ls100")
        add("head_batch", B=5, P=1, D=D, K=4, mode="given", recipe="parallel")
        add("head_batch", B=5, P=1, D=D, K=4, mode="given", adapter=False, recipe="zero_pooled")
    # -- vlsa_head_forward_batch_text: B from 1; the text rows of norm 1e3 / 1e-6 matter here (the launch normalises them)
    for i, B in enumerate((1, 2, 9, 16, 17, 33, 65)):
        for D in (512, _rot((252, 768, 4, 1020, 516, 12, 1024), i)):
            add("head_batch_text", B=B, P=_rot(QUERIES, i + 1), D=D, K=_rot(RANKS, i + 2 + (D == 512)), mode=_rot(MODES, i),
                adapter=not (i % 3 == 2 and D != 512), inc=i % 2 == 0)
    for i, B in enumerate(BAGS):                       # every B, the widths 256 / 508 / 1020 among them
        add("head_batch_text", B=B, P=_rot(QUERIES, i), D=_rot((256, 508, 1020, 512), i), K=_rot(RANKS, i + 3), mode=_rot(MODES, i + 1),
            adapter=i % 5 != 4, bias=i % 2 == 0, recipe="randn")
    add("head_batch_text", B=17, P=2, D=512, K=17, mode="mean", adapter=False)
    add("head_batch_text", B=9, P=2, D=768, K=4, mode="mean", adapter=False)
    for D, B in ((516, 9), (512, 17)):
        for r in FWD_RECIPES:
            add("head_batch_text", **_recipe_fields(r, dict(B=B, P=12, D=D, K=4)))
    # -- vlsa_vlfan_merge_head: every G fused (D = 512, adapter, mean / weight) and unfused (max, identity, another width)
    for i, G in enumerate(G_SINGLE):
        add("merge_head", G=G, P=_rot(QUERIES, i), K=_rot(RANKS, i), mode=("mean", "weight")[i % 2], bias=i % 3 != 0, inc=i % 4 != 3)
        add("merge_head", G=G, P=_rot(QUERIES, i + 1), K=_rot(RANKS, i + 1), mode=_rot(("max", "mean", "weight"), i), adapter=i % 3 == 0 and i % 2 == 0)
        add("merge_head", G=G, P=_rot(QUERIES, i + 2), D=_rot((256, 768, 1024, 8), i), K=_rot(RANKS, i + 2), mode=_rot(MODES, i))
    for G, D, a in ((1, 512, True), (17, 512, False), (257, 768, True), (512, 512, True)):     # given pooling: row 0 of the merged rows, unfused
        add("merge_head", G=G, P=_rot((1, 12), G), D=D, K=4, mode="given", adapter=a)
    for G in (3, 17, 257, 512):
        for r in MERGE_RECIPES:
            add("merge_head", G=G, P=12, K=4, recipe=r)                                   # fused
            add("merge_head", G=G, P=12, K=4, mode="max", recipe=r)                       # unfused
    for r in ("parallel", "sat_weight", "norm1e3", "norm1e-6"):
        add("merge_head", **_recipe_fields(r, dict(G=17, P=12, K=4)))
    # -- vlsa_vlfan_merge_head_batch_strided: every G contiguous and strided, the switch (G = 8 / 9) at P 1 / 16 under max / weight,
    #    widths other than 512, empty records
    for i, G in enumerate(G_BATCH):
        for lay in ("contig", "strided"):
            s = lay == "strided"
            add("merge_head_batch", B=_rot((2, 7, 17, 1, 9), i + s), G=G, P=_rot(QUERIES, i + s), D=_rot((512, 252, 516, 512, 1024, 12, 768, 4), i + 3 * s),
                K=_rot(RANKS, i + s), mode=_rot(MODES, i + s), layout=lay, adapter=(i + s) % 4 != 3, bias=i % 3 != 1, inc=(i + s) % 3 != 0)
    add("merge_head_batch", B=9, G=7, P=2, D=1020, K=4, mode="mean")
    add("merge_head_batch", B=17, G=10, P=12, D=1020, K=17, mode="weight", layout="strided")
    for G in (8, 9):
        for P in (1, 16):
            for mode in ("max", "weight"):
                add("merge_head_batch", B=3, G=G, P=P, D=_rot((512, 508), P), K=4, mode=mode, layout=("strided", "contig")[G - 8])
        add("merge_head_batch", B=17, G=G, P=12, D=512, K=17, mode="mean")                # MFMA + in-place finish
        add("merge_head_batch", B=16, G=G, P=2, D=512, K=16, mode="mean", layout="strided")
        add("merge_head_batch", B=9, G=G, P=2, D=256, K=4, mode="mean", adapter=False)
        add("merge_head_batch", B=9, G=G, P=2, D=252, K=17, mode="mean", adapter=False)
    for G in (3, 8, 9, 33):
        for r in MERGE_RECIPES:
            add("merge_head_batch", B=3, G=G, P=12, D=_rot((512, 516), G), K=4, layout=("contig", "strided")[G % 2], recipe=r)
    # -- vlsa_head_backward_batch: every B with and without the adapter over the widths (and D = 2, 33: any D >= 1 is accepted)
    for i, B in enumerate(BAGS):
        for a in (True, False):
            add("head_backward", B=B, P=_rot(QUERIES, i + a), D=_rot(WIDTHS, i + 3 * a), K=_rot(RANKS, i + a), adapter=a, gv=(i + a) % 2 == 0,
                gt=(i // 2 + a) % 2 == 0)
    for B, D in ((65, 512), (129, 252), (128, 516), (64, 508), (72, 768), (129, 1024), (128, 256)):
        add("head_backward", B=B, P=2, D=D, K=4, adapter=True, gv=B % 2 == 1, gt=D % 8 == 0)     # the dW / db carry across chunks of 64
    for D in (2, 33):          # (D = 1 is accepted too, but x / |x| is constant there: every gradient through a normalisation is rounding noise)
        for a in (True, False):
            add("head_backward", B=9, P=2, D=D, K=4, adapter=a, gv=True, gt=True)
    for B, D in ((16, 512), (9, 256), (8, 1024)):
        add("head_backward", B=B, P=12, D=D, K=4, adapter=False)
    for gv in (False, True):
        for gt in (False, True):
            add("head_backward", B=17, P=12, D=516, K=17, gv=gv, gt=gt)
    for B, D in ((9, 516), (70, 512)):
        for r in BWD_RECIPES:
            add("head_backward", **_recipe_fields(r, dict(B=B, P=12, D=D, K=4, gv=r != "dl_zero", gt=r not in ("dl_zero", "dl_onehot"))))
        add("head_backward", B=B, P=12, D=D, K=4, ls=0.0)
        add("head_backward", B=B, P=12, D=D, K=17, ls=LS_100, recipe="ls100")
    # -- VF.head_train: P = 1 as vlsa.py calls it, and P = 12 with the adapter
    for B, D, a in ((1, 256, False), (1, 768, False), (1, 512, True), (9, 256, False), (9, 768, True), (2, 512, False), (17, 1020, True)):
        add("head_train", B=B, P=12 if a else 1, D=D, K=4 if D != 768 else 17, adapter=a)
    # -- vlsa_query_chain (17 ungated queries: the entry accepts nq <= 17 either way, vlsa_prepare_queries at most 16 effective ones, so no
    #    caller of the library reaches it; the block is filled in by hand for that case, as for the widths D % 8 != 0 the preparation refuses)
    for i, (nq, gated) in enumerate(((1, False), (2, False), (13, False), (17, False), (2, True), (13, True), (17, True))):
        for D in (512, _rot((4, 252, 516, 1024, 12, 768, 1020), i)):
            add("query_chain", P=nq - gated, nq=nq, gated=gated, D=D)
        add("query_chain", P=nq - gated, nq=nq, gated=gated, D=508, recipe="norm1e3")
        add("query_chain", P=nq - gated, nq=nq, gated=gated, D=256, recipe="norm1e-6")
    return cs


CASES = _build_cases()


def cases_of(entry):
    return [c for c in CASES if c.entry == entry]


# ---- refusals: (entry, what, overrides) -- each must answer VLSA_EINVAL before anything is launched -----------------------------------
REFUSALS = [
    ("head_forward", "D % 4", dict(D=510)), ("head_batch", "D % 4", dict(D=510, B=3)), ("head_batch_text", "D % 4", dict(D=510, B=3)),
    ("merge_head_batch", "D % 4", dict(D=510, B=3, G=2)),
    ("merge_head", "D % 8", dict(D=508, G=3)),
    ("head_forward", "D > 1024", dict(D=1028)), ("head_batch", "D > 1024", dict(D=1028, B=3)), ("head_batch_text", "D > 1024", dict(D=1028, B=3)),
    ("merge_head", "D > 1024", dict(D=1032, G=3)), ("merge_head_batch", "D > 1024", dict(D=1028, B=3, G=2)),
    ("head_backward", "D > 1024", dict(D=1028, B=3)), ("query_chain", "D > 1024", dict(D=1028, nq=3)),
    ("head_forward", "P > 16", dict(P=17)), ("head_batch", "P > 16", dict(P=17, B=3)), ("head_batch_text", "P > 16", dict(P=17, B=3)),
    ("merge_head", "P > 16", dict(P=17, G=3)), ("merge_head_batch", "P > 16", dict(P=17, B=3, G=2)), ("head_backward", "P > 16", dict(P=17, B=3)),
    ("query_chain", "nq > 17", dict(nq=18)), ("query_chain", "gated nq = 1", dict(nq=1, gated=True)),
    ("head_forward", "K > 64", dict(K=65)), ("head_batch", "K > 64", dict(K=65, B=3)), ("head_batch_text", "K > 64", dict(K=65, B=3)),
    ("merge_head", "K > 64", dict(K=65, G=3)), ("merge_head_batch", "K > 64", dict(K=65, B=3, G=2)), ("head_backward", "K > 64", dict(K=65, B=3)),
    ("head_forward", "weight without pool_w", dict(mode="weight", P=4, pool_w=False)),
    ("head_batch", "weight without pool_w", dict(mode="weight", P=4, B=3, pool_w=False)),
    ("head_batch_text", "weight without pool_w", dict(mode="weight", P=4, B=3, pool_w=False)),
    ("merge_head", "weight without pool_w", dict(mode="weight", P=4, G=3, pool_w=False)),
    ("merge_head_batch", "weight without pool_w", dict(mode="weight", P=4, B=3, G=2, pool_w=False)),
    ("head_batch_text", "pooled == rows", dict(B=3, P=1, layout="inplace")),
    ("head_batch_text", "given pooling", dict(B=3, P=1, mode="given")),
    ("merge_head_batch", "given pooling", dict(B=3, G=2, P=1, mode="given")),
    ("merge_head_batch", "stride % 4", dict(B=3, G=2, P=2, strides_ok=False)),
]


def refusal_path(entry, kw):
    kw = dict(kw)
    return expected_path(entry, **kw)


# ---- input recipes ------------------------------------------------------------------------------------------------------------------
def _gen(c, salt=0):
    return torch.Generator().manual_seed((zlib.crc32(c.id.encode()) ^ 0x5bd1e995) + salt)


def pool64(rows, mode, pw):
    """[B, P, D] float64 -> pooled [B, D]"""
    if mode == "mean":
        return rows.mean(dim=1)
    if mode == "max":
        return rows.max(dim=1).values
    if mode == "weight":
        return (torch.softmax(pw.double(), 0)[None, :, None] * rows).sum(dim=1)
    return rows[:, 0]


def merge64(pm, pl, pacc, P):
    """pm, pl [B, G, 16], pacc [B, G, P, D] (any float dtype) -> m2 [B, P], l [B, P], out [B, P, D] in float64: the log2-domain
    log-sum-exp merge; a record whose max is -inf weighs 0"""
    pm, pl, pacc = pm.double()[..., :P], pl.double()[..., :P], pacc.double()
    m2 = pm.max(dim=1).values
    f = torch.exp2(pm - m2[:, None])                       # exp2(-inf) = 0
    l = (pl * f).sum(dim=1)
    out = (pacc * f[..., None]).sum(dim=1) / l[..., None]
    return m2, l, out


def make_inputs(c):
    """fp32 CPU tensors by the case's recipe, one seeded generator per case.
      randn        standard normal rows, W ~ N(0, 1 / D), b ~ 0.1 N, raw text rows 3 N, pool_w N
      parallel     text row 0 is the bag vector of bag 0 plus 1e-3 of noise, row 1 (K > 1) its negative: logits near +-exp(ls), where
                   v^ - v^ (v^ . dv^) cancels worst
      norm1e3      rows and raw text rows scaled by 1e3;       norm1e-6: by 1e-6
      zero_pooled  every row of bag 0 is zero, identity adapter: the 1e-12 clamp, forward and backward
      max_ties     max pooling: rows 0 and 1 of every bag agree in the even columns
      sat_weight   one entry of pool_w is 40 above the rest: the softmax saturates
      ls100        logit_scale = log 100 (Case.ls; ls = 0 cases carry it in Case.ls too)
      dl_onehot    dlogits zero but for one entry of one bag;  dl_zero: all zero (and no g_vhat / g_That)
      empty_first / _middle / _last   that partial record of every bag is (-inf, 0, 0);   spread60: record maxima uniform in +-60
    """
    g = _gen(c)
    B, P, D, K = c.B, c.P, c.D, c.K
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    inp = {"ls": torch.tensor([c.ls], dtype=torch.float32)}
    if c.entry == "query_chain":
        Q, dE = rn(c.nq, D), rn(P, D)
        if c.recipe == "norm1e3":
            Q *= 1e3
        elif c.recipe == "norm1e-6":
            Q *= 1e-6
        inp.update(Q=Q, dE=dE)
        return inp
    if c.entry in ("merge_head", "merge_head_batch"):
        G = c.G
        pm, pl, pacc = rn(B, G, P_STRIDE) * 20, torch.rand(B, G, P_STRIDE, generator=g) + 0.5, rn(B, G, P, D)
        if c.recipe == "spread60":
            pm = (torch.rand(B, G, P_STRIDE, generator=g) * 2 - 1) * 60
        if c.recipe.startswith("empty_"):
            gi = {"empty_first": 0, "empty_middle": G // 2, "empty_last": G - 1}[c.recipe]
            pm[:, gi], pl[:, gi], pacc[:, gi] = float("-inf"), 0.0, 0.0
        inp.update(pm=pm, pl=pl, pacc=pacc)
        rows = merge64(pm, pl, pacc, P)[2]
    else:
        rows = rn(B, P, D)
    W = rn(D, D) * D ** -0.5 if c.adapter else None
    b = rn(D) * 0.1 if c.adapter and c.bias else None
    T = rn(K, D) * 3
    pw = rn(P) if c.mode == "weight" else None
    if c.recipe == "norm1e3":
        rows, T = rows * 1e3, T * 1e3
    elif c.recipe == "norm1e-6":
        rows, T = rows * 1e-6, T * 1e-6
    elif c.recipe == "zero_pooled":
        rows[0] = 0.0
    elif c.recipe == "max_ties":
        rows[:, 1, 0::2] = rows[:, 0, 0::2]
    elif c.recipe == "sat_weight":
        pw[P // 2] = pw.max() + 40.0
    if c.recipe in ("norm1e3", "norm1e-6") and "pacc" in inp:
        inp["pacc"] = inp["pacc"] * (1e3 if c.recipe == "norm1e3" else 1e-6)
    if c.recipe == "parallel":
        pooled = pool64(rows.double() if rows.dtype != torch.float64 else rows, c.mode, pw)
        v = pooled if W is None else pooled @ W.double().t() + (0 if b is None else b.double())
        T[0] = (v[0] / v[0].norm()).float() * 3 + 3e-3 * rn(D) / D ** 0.5
        if K > 1:
            T[1] = -(v[0] / v[0].norm()).float() * 3 + 3e-3 * rn(D) / D ** 0.5
    if "pacc" not in inp:
        inp["rows"] = rows.float()
    inp.update(W=W, b=b, T=T, pw=pw)
    # the unit text rows the forward entries read (F.normalize in fp32: what VF.normalize_rows hands them, to an ulp)
    inp["That"] = TF.normalize(T, dim=-1)
    if c.entry == "head_backward":
        dl = rn(B, K)
        if c.recipe == "dl_onehot":
            dl = torch.zeros(B, K)
            dl[B // 2, K // 2] = 1.0
        elif c.recipe == "dl_zero":
            dl = torch.zeros(B, K)
        inp.update(dlogits=dl, g_vhat=rn(B, D) if c.gv else None, g_That=rn(K, D) if c.gt else None)
    if c.entry == "head_train":
        inp.update(dlogits=rn(B, K), g_vhat=rn(B, D), g_That=rn(K, D))
    return inp


def strided_layout(c):
    """strides9 (floats) of a merge_head_batch case and the buffer sizes: {partial stride of pm, pl, pacc; bag stride of pm, pl, pacc;
    bag stride of m2, l, out}.  "strided": spare floats between records and between bags (multiples of 4 where the ABI asks)."""
    G, P, D = c.G, c.P, c.D
    if c.layout == "strided":
        sm, sl, sa = P_STRIDE + 3, P_STRIDE + 5, P * D + 8
        bm, bl, ba = G * sm + 7, G * sl + 2, G * sa + 12
        om, ol, oo = P_STRIDE + 1, P_STRIDE + 6, P * D + 4
    else:
        sm, sl, sa = P_STRIDE, P_STRIDE, P * D
        bm, bl, ba = G * sm, G * sl, G * sa
        om, ol, oo = P_STRIDE, P_STRIDE, P * D
    return [sm, sl, sa, bm, bl, ba, om, ol, oo]


# ---- float64 references and torch's fp32 evaluation of the same formulas ------------------------------------------------------------
def _forward(c, inp, dt):
    """the tail in dtype ``dt`` from the values the kernels read; text: the unit rows given (That), or the raw rows (batch_text / head_train)"""
    out = {}
    cast = lambda t: None if t is None else t.to(dt)  # noqa: E731
    if "pacc" in inp:
        if dt == torch.float64:
            m2, l, rows = merge64(inp["pm"], inp["pl"], inp["pacc"], c.P)
        else:
            pm, pl = inp["pm"][..., :c.P], inp["pl"][..., :c.P]
            m2 = pm.max(dim=1).values
            f = torch.exp2(pm - m2[:, None])
            l = (pl * f).sum(dim=1)
            rows = (inp["pacc"] * f[..., None]).sum(dim=1) / l[..., None]
        out.update(m2=m2, l=l, out=rows)
    else:
        rows = cast(inp["rows"])
    pooled = pool64(rows, c.mode, inp["pw"]) if dt == torch.float64 else _pool32(rows, c.mode, inp["pw"])
    W, b = cast(inp["W"]), cast(inp["b"])
    v = pooled if W is None else pooled @ W.t() + (0 if b is None else b)
    vnorm = v.norm(dim=-1, keepdim=True).clamp_min(NORM_EPS)
    vhat = v / vnorm
    if c.entry in ("head_batch_text", "head_train"):
        T = cast(inp["T"])
        tnorm = T.norm(dim=-1, keepdim=True).clamp_min(NORM_EPS)
        That = T / tnorm
        out.update(That=That, tnorm=tnorm[:, 0])
    else:
        That = cast(inp["That"])
    logits = cast(inp["ls"]).exp() * vhat @ That.t()
    out.update(pooled=pooled, v=v, vhat=vhat, vnorm=vnorm[:, 0], logits=logits)
    if c.inc:
        out["incidence"] = torch.softmax(logits, dim=-1)
    return out


def _pool32(rows, mode, pw):
    if mode == "mean":
        return rows.mean(dim=1)
    if mode == "max":
        return rows.max(dim=1).values
    if mode == "weight":
        return (torch.softmax(pw, 0)[None, :, None] * rows).sum(dim=1)
    return rows[:, 0]


def _backward(c, inp, dt):
    """gradients of sum(dlogits logits) + sum(g_vhat v^) + sum(g_That T^) by torch autograd in dtype ``dt``: mean pooling, adapter,
    F.normalize with its 1e-12 clamp (a zero vector: d v = g / 1e-12, the norm's subgradient 0), raw text rows, pre-exp logit scale"""
    leaf = lambda t: None if t is None else t.to(dt).clone().requires_grad_(True)  # noqa: E731
    rows, W, T, ls = leaf(inp["rows"]), leaf(inp["W"]), leaf(inp["T"]), leaf(inp["ls"])
    b = leaf(inp["b"])
    pooled = rows.mean(dim=1)
    v = pooled if W is None else pooled @ W.t() + (0 if b is None else b)
    vhat = v / v.norm(dim=-1, keepdim=True).clamp_min(NORM_EPS)
    That = T / T.norm(dim=-1, keepdim=True).clamp_min(NORM_EPS)
    logits = ls.exp() * vhat @ That.t()
    loss = (inp["dlogits"].to(dt) * logits).sum()
    if inp.get("g_vhat") is not None:
        loss = loss + (inp["g_vhat"].to(dt) * vhat).sum()
    if inp.get("g_That") is not None:
        loss = loss + (inp["g_That"].to(dt) * That).sum()
    loss.backward()
    out = {"drows": rows.grad, "dT": T.grad, "dls": ls.grad}
    if W is not None:
        out["dW"] = W.grad
        # (the kernel always writes db; without a bias parameter it is the gradient a zero bias would get)
        out["db"] = b.grad if b is not None else _db_without_bias(c, inp, dt)
    fw = {"pooled": pooled.detach(), "vhat": vhat.detach(), "vnorm": v.detach().norm(dim=-1).clamp_min(NORM_EPS), "That": That.detach(),
          "tnorm": T.detach().norm(dim=-1).clamp_min(NORM_EPS), "logits": logits.detach()}
    return out, fw


def _db_without_bias(c, inp, dt):
    inp2 = dict(inp, b=torch.zeros(c.D))
    return _backward(c, inp2, dt)[0]["db"]


def _query_chain(c, inp, dt):
    Q = inp["Q"].to(dt).clone().requires_grad_(True)
    qhat = Q / Q.norm(dim=-1, keepdim=True).clamp_min(NORM_EPS)
    e = qhat[:c.P] - qhat[c.P] if c.gated else qhat
    (e * inp["dE"].to(dt)).sum().backward()
    return {"dQ": Q.grad}


def evaluate(c, inp, dt):
    """{output name: tensor} of a case in dtype ``dt``: float64 is the reference, float32 torch-CPU's own evaluation"""
    if c.entry == "query_chain":
        return _query_chain(c, inp, dt)
    if c.entry == "head_backward":
        return _backward(c, inp, dt)[0]
    if c.entry == "head_train":
        g, fw = _backward(c, inp, dt)
        g.pop("db") if (c.adapter and not c.bias) else None
        return dict(g, logits=fw["logits"], vhat=fw["vhat"], That=fw["That"])
    return _forward(c, inp, dt)


def reference(c, inp):
    return evaluate(c, inp, torch.float64)


def fp32_eval(c, inp):
    return evaluate(c, inp, torch.float32)


def backward_saved(c, inp):
    """the forward's outputs vlsa_head_backward_batch reads, rounded from float64 to fp32 (what a correct forward hands over)"""
    return {k: v.float() for k, v in _backward(c, inp, torch.float64)[1].items()}


_SCALED = ("pooled", "v", "out", "vnorm", "tnorm")      # outputs that shrink with the rows and text rows of the norm1e-6 recipe


def gate(c, name, ref):
    """absolute tolerance of output ``name`` of case ``c`` against (a part of) its float64 reference tensor.  The rows-kind gate
    1e-4 x max(1, max|ref|) would leave the 1e-6-sized outputs of the norm1e-6 recipe unchecked, so there it is 1e-4 of the reference's
    largest entry, the rule of the gradients (fp32 rounding is relative: torch's fp32 evaluation stays below 0.01 of it)."""
    if name in _ABS:
        return _ABS[name]
    big = float(ref.abs().max()) if ref.numel() else 0.0
    if name in _GRADS or (c.recipe == "norm1e-6" and name in _SCALED):
        return GATE_GRAD * big
    return GATE_ROWS * max(1.0, big)


def _parts(c, name, ref):
    """the slices of an output that are judged on their own: under zero_pooled the row gradient of bag 0 is g / 1e-12, and a gate
    taken from the whole tensor's largest entry would leave every other bag unchecked"""
    if c.recipe == "zero_pooled" and name == "drows" and ref.shape[0] > 1:
        return [(" [bag 0]", slice(0, 1)), (" [bags 1..]", slice(1, None))]
    return [("", slice(None))]


def judged(c, got, ref):
    """[(output label, error, gate)] of a case's outputs ``got`` against the float64 reference ``ref``"""
    out = []
    for name, r in ref.items():
        g = got[name].detach().double().cpu().reshape(r.shape)
        for label, idx in _parts(c, name, r):
            out.append((name + label, err_of(g[idx], r[idx]), gate(c, name, r[idx])))
    return out


def err_of(got, ref):
    d = (got.double().reshape(ref.shape) - ref).abs()
    return float(d.max()) if d.numel() else 0.0


def ratio(err, g):
    """error in units of its gate (a zero gate -- an identically zero gradient -- is met by an exact zero only)"""
    if not err == err:
        return float("inf")
    return err / g if g > 0 else (0.0 if err == 0 else float("inf"))
