"""Sentence shapes at which the text tower (vlsa_amd/csrc/text_tower.hip) takes another path, for the CLIP towers: QuickGELU
(``VLSA_TT_ACT_QUICK_GELU``) and the <eot> row pooled, no CLS token (``VLSA_TT_POOL_LAST_TOKEN``).  The counterpart of
tests/text_shape_cases.py, whose helpers (``assemble``, ``per_prompt_rel``, ``tensor_rel``, the gates) it shares.

tests/test_gpu_clip_text.py holds the CLIP towers at widths 128 and 512 (runtime-G products), on equal-length rank prompts behind a
prefix of 1 .. 5 positions.  The table below is the CoCa sweep's, restated for a 77-position tower at width 768: one case on each side
of every threshold the host code branches on.  tests/test_clip_shape_cases_cpu.py pins the (M, M_pad, max_len, prefix_len, kpb) columns
to ``last_token_rows`` so that an edit cannot move a case off its boundary unnoticed, and tests/test_gpu_clip_text_shapes.py runs every
case against the float64 truth (``clip_text_helpers.clip_text_forward``).  Imports without a GPU.

A prompt whose <eot> sits at position m has m + 1 rows (positions 0 .. m, the last one pooled): ``pseudo[i, :m + 1] = 1 .. m + 1``.

What the host code decides from a case's numbers (width 768, 12 heads; PRO + 4 = the QuickGELU variant of a GELU-epilogue product):
    in_proj product     M <= 112: 16 x 64 tiles  k_tt_gemm<1, 4, 1, 12, 4> | <= 160: 32 x 48  <2, 4, 1, 12, 3> | else 48 x 48  <3, 4, 1, 12, 3>
    c_fc product        M <= 128: 16 x 96 tiles  k_tt_gemm<1, 4, 5, 12, 6> | <= 160: 32 x 64  <2, 4, 5, 12, 4> | else 48 x 48  <3, 4, 5, 12, 3>
    d h_pre product     the same three tiles: <1, 4, 4, 12, 6> | <2, 4, 4, 12, 4> | <3, 4, 4, 12, 3>
    frozen backward     M <= 128: LayerNorm backward as a product prologue -- d h_pre below the top block is k_tt_gemm<1, 4, 6, 12, 6> --
                        and d prompts_embedding written by the last k_tt_ln_bwd4 | else one launch per stage
    M_pad               whole 96-row groups: 96 -> 96, 97 -> 192
    prefix keys         keys per key workgroup = the fewest kpb in 1 .. 4 with (K + 1 + ceil(L / kpb)) * heads <= 256, and only when
                        M <= 128; else the ticketed fold (``kpb`` 0 below).  The kernel's names do not show kpb; ``keys_per_workgroup``
                        restates the arithmetic and the CPU test holds the column to it.
    attention           a wave per row of the longest prompt, 4 .. 16 waves; the forward takes a second key chunk at S > 64; the backward
                        refuses max_len > 64.
    d pooled            out_dim 512: k_tt_gemm<1, 4, 0, 8, 1> on the incoming gradient as it lies | out_dim 768: k_tt_tile_rows +
                        k_tt_gemm<3, 4, 0, 0, 2>
"""
from __future__ import annotations

import functools
import os
import sys
import zlib
from collections import namedtuple

import torch

if __name__ == "__main__":      # run as a script (the seed search below): what tests/conftest.py puts on the path
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(_here), os.path.join(_here, "golden")]

import clip_text_cases as CC
from text_shape_cases import GATE, YARDSTICK_MAX, assemble, per_prompt_rel, tensor_rel  # noqa: F401  (the same gates and measures)

CTX = CC.CTX
# tower -> weight seed (all in CC.WEIGHT_SCALES at (3.5, 3.5): attention rows peaked, QuickGELU inputs past |6|)
TOWER_SEEDS = {"w768x2": 9141, "w768x3": 9142, "w768x2_o768": 9143}

# name, tower, rows per prompt (<eot> position + 1), L asked for; then what last_token_rows must answer: M, M_pad, max_len, prefix_len;
# kpb: prefix keys per key workgroup of the attention backward (None: no prefix in the plan, 0: ticketed fold);
# route: the frozen tower's backward ("fused": PRO_LNBWD prologues, "stage": a launch per stage, None: forward only)
ShapeCase = namedtuple("ShapeCase", "name tower rows L M M_pad max_len prefix_len kpb route")


def _c(name, tower, rows, L, M, M_pad, max_len, prefix_len, kpb, route):
    return ShapeCase(name, tower, tuple(rows), L, M, M_pad, max_len, prefix_len, kpb, route)


CASES = [
    # ---- ragged prompts and the attention kernels' row loops (no prefix) ------------------------------------------------
    _c("ragged100", "w768x2", [3, 16, 17, 64], 0, 100, 192, 64, 0, None, "fused"),       # an exact 64-row prompt in the backward
    _c("ragged154", "w768x2", [3, 4, 16, 17, 18, 32, 64], 0, 154, 192, 64, 0, None, "stage"),
    _c("one", "w768x2", [13], 0, 13, 96, 13, 0, None, "fused"),                          # a single prompt
    _c("sot_eot", "w768x2", [2, 13], 0, 15, 96, 13, 0, None, "fused"),                   # <sot><eot> alone, with a gradient
    # ---- forward only: S = 64, 65, 66 (the second key chunk's first key, then one some OTHER row attends to), 77, 2 -----
    _c("fwd_edges", "w768x2", [64, 65, 66, 77, 2], 0, 274, 288, 77, 0, None, None),
    # ---- the row thresholds ---------------------------------------------------------------------------------------------
    _c("M96", "w768x2", [16] * 6, 0, 96, 96, 16, 0, None, "fused"),
    _c("M97", "w768x2", [16] * 5 + [17], 0, 97, 192, 17, 0, None, "fused"),
    _c("M112", "w768x2", [14] * 8, 0, 112, 192, 14, 0, None, "fused"),
    _c("M113", "w768x2", [14] * 7 + [15], 0, 113, 192, 15, 0, None, "fused"),
    _c("M128", "w768x2", [16] * 8, 0, 128, 192, 16, 0, None, "fused"),
    _c("M129", "w768x2", [16] * 7 + [17], 0, 129, 192, 17, 0, None, "stage"),
    _c("M160", "w768x2", [16] * 10, 0, 160, 192, 16, 0, None, "stage"),
    _c("M161", "w768x2", [16] * 9 + [17], 0, 161, 192, 17, 0, None, "stage"),
    # ---- shared prefix, K = 12: (K + 1 + ceil(L / kpb)) * 12 <= 256; M = L + sum(r - L) ----------------------------------
    _c("L8", "w768x2", [13] * 12, 8, 68, 96, 13, 8, 1, "fused"),              # 8 key workgroups per head
    _c("L9", "w768x2", [14] * 12, 9, 69, 96, 14, 9, 2, "fused"),              # 5 groups, the last holds one key
    _c("L17", "w768x2", [22] * 12, 17, 77, 96, 22, 17, 3, "fused"),           # 6 groups, the last holds two
    _c("L25", "w768x2", [30] * 12, 25, 85, 96, 30, 25, 4, "fused"),           # 7 groups, the last holds one
    _c("L33", "w768x2", [38] * 12, 33, 93, 96, 38, 33, 0, "fused"),           # no kpb <= 4 fits: ticket at M <= 128
    _c("L8M128", "w768x2", [18] * 12, 8, 128, 192, 18, 8, 1, "fused"),
    _c("L8M129", "w768x2", [18] * 11 + [19], 8, 129, 192, 19, 8, 0, "stage"),             # M > 128: ticket
    _c("S64pfx", "w768x2", [64, 64], 25, 103, 192, 64, 25, 2, "fused"),                   # (2 + 1 + 13) * 12 = 192; S = 64 with the prefix
    _c("K16L17", "w768x2", [20] * 16, 17, 65, 96, 20, 17, 0, "fused"),                    # (17 + 5) * 12 > 256 at kpb 4: ticket, 17 shares per key
    _c("raggedpfx", "w768x2", [11, 12, 16, 32, 11, 14], 9, 51, 96, 32, 9, 1, "fused"),    # (6 + 1 + 9) * 12 = 192; 2 .. 23 own rows
    _c("fallback", "w768x2", [13] * 5 + [8], 8, 73, 96, 13, 0, None, "fused"),            # a prompt ends inside the prefix: planned with L = 0
    # ---- three blocks: one that is neither top nor bottom ----------------------------------------------------------------
    _c("x3_L9", "w768x3", [14] * 12, 9, 69, 96, 14, 9, 2, "fused"),
    # ---- ViT-L/14's projection: the d pooled product's other branch --------------------------------------------------------
    _c("o768_ragged100", "w768x2_o768", [3, 16, 17, 64], 0, 100, 192, 64, 0, None, "fused"),
]
BY_NAME = {c.name: c for c in CASES}

# outside the table above: the HuggingFace layout under a prefix plan (same columns)
EXTRA = {c.name: c for c in [
    _c("o768_L9", "w768x2_o768", [14] * 12, 9, 69, 96, 14, 9, 2, "fused"),
]}
# what the trainable tower runs (every weight a leaf in the truth)
TRAIN_CASES = ["ragged100", "L9", "L25", "ragged154"]
# the HuggingFace layout on w768x2_o768: case, hidden_act
HF_CASES = [("o768_ragged100", "quick_gelu"), ("o768_L9", "quick_gelu"), ("o768_ragged100", "gelu")]
# the cases the CPU test holds to the condition on the inputs (fp32 truth within a quarter of the gate of the float64 one)
CONDITION_CASES = ["ragged100", "L9", "S64pfx"]
# The embeddings' seed is crc32(case name) + SEED_STEP[name]: the rule of text_shape_cases.SEED_STEP, which never looks at the GPU.  The
# step is the FIRST in 0 .. 11 at which the fp32 CPU truth stays within YARDSTICK_MAX of the float64 one by the GPU test's measures
# (features absolute, d own rows per prompt, d prefix per tensor), else the step in 0 .. 11 where that distance is smallest
# (`python tests/clip_shape_cases.py` prints the search).  Inputs on which plain fp32 misses the gate by itself say nothing about a kernel.
# With in_proj / c_fc scaled by 3.5 the fp32 truth's distance is 0.7e-5 .. 6e-5 depending on the draw.
# No step in 0 .. 11 meets the condition for L25 (3.0e-5 at step 1), L33 (3.0e-5 at step 8), K16L17 (3.1e-5 at step 6) and
# x3_L9 (3.3e-5 at step 8).
SEED_STEP = {"ragged100": 1, "ragged154": 6, "M96": 3, "M113": 2, "M128": 1, "M129": 2, "M160": 1, "L8": 2, "L9": 9, "L17": 8, "L25": 1,
             "L33": 8, "S64pfx": 5, "K16L17": 6, "raggedpfx": 2, "x3_L9": 8, "o768_L9": 3}


def get(name) -> ShapeCase:
    return BY_NAME[name] if name in BY_NAME else EXTRA[name]


def keys_per_workgroup(case: ShapeCase):
    """The attention backward's choice for the prefix keys, restated from tt_backward: None without a prefix, 0 = ticketed fold."""
    if case.prefix_len == 0:
        return None
    heads, K, L = CC.TOWERS[case.tower]["heads"], len(case.rows), case.prefix_len
    if case.M <= 128 and heads <= 16:
        for kpb in (1, 2, 3, 4):
            if (K + 1 + -(-L // kpb)) * heads <= 256:
                return kpb
    return 0


def route_of(case: ShapeCase):
    """The frozen backward's route at width 768, restated from tt_backward's ``fuse``: 16 x 96 and 16 x 32 tiles within one round of CUs."""
    rt = -(-case.M // 16)
    return "fused" if rt * 32 <= 256 and rt * 24 <= 256 else "stage"


def pseudo_tokens(rows) -> torch.Tensor:
    """[K, 77]: 1 .. r in front (the largest on the <eot> slot), zeros behind"""
    out = torch.zeros(len(rows), CTX, dtype=torch.long)
    for s, r in enumerate(rows):
        out[s, :r] = torch.arange(1, r + 1)
    return out


@functools.lru_cache(maxsize=None)
def make_weights(tower: str):
    """the tower's seeded fp32 weights (cached: treat as read-only)"""
    return CC.make_clip_weights(tower, TOWER_SEEDS[tower])


def make_inputs(case: ShapeCase):
    """Seeded N(0, 0.02^2) embeddings (no learner in between): ``prefix`` [L, d] (None without one) and ``own`` [K, 77 - L, d], the two
    leaves of a shared-prefix case; ``pseudo`` [K, 77]; ``G`` [K, out_dim], the seeded weights of the scalar that is differentiated."""
    c = CC.TOWERS[case.tower]
    g = torch.Generator().manual_seed((zlib.crc32(case.name.encode()) + SEED_STEP.get(case.name, 0)) & 0x7FFFFFFF)
    K, d, L = len(case.rows), c["width"], case.L
    prefix = torch.randn(L, d, generator=g) * 0.02 if L > 0 else None
    own = torch.randn(K, CTX - L, d, generator=g) * 0.02
    G = torch.randn(K, c["out_dim"], generator=g)
    return dict(prefix=prefix, own=own, pseudo=pseudo_tokens(case.rows), G=G)


def truth(case: ShapeCase, inp, dtype=torch.float64, weight_grads=False, backward=True, act="quick_gelu"):
    """``clip_text_forward`` over the full 77 positions in ``dtype`` under autograd.
    -> dict(feats, d_prefix, d_own, d_emb [K, 77, d], d_w {name: grad}, stats)."""
    import clip_text_helpers as CH
    c = CC.TOWERS[case.tower]
    W = {k: v.to(dtype) for k, v in make_weights(case.tower).items()}
    if weight_grads:
        W = {k: v.clone().requires_grad_(k != "token_embedding.weight") for k, v in W.items()}
    prefix = inp["prefix"].to(dtype).requires_grad_(backward) if inp["prefix"] is not None else None
    own = inp["own"].to(dtype).requires_grad_(backward)
    emb = assemble(prefix, own)
    stats = {}
    with torch.set_grad_enabled(backward):
        feats = CH.clip_text_forward(W, c["heads"], emb, inp["pseudo"], c["layers"], act, stats)
    out = dict(feats=feats.detach(), d_prefix=None, d_own=None, d_emb=None, d_w=None, stats=stats)
    if backward:
        if prefix is not None:
            emb.retain_grad()
        (feats * inp["G"].to(dtype)).sum().backward()
        out.update(d_prefix=None if prefix is None else prefix.grad, d_own=own.grad, d_emb=emb.grad)
        if weight_grads:
            out["d_w"] = {k: v.grad for k, v in W.items() if k != "token_embedding.weight"}
    return out


def yardstick(case: ShapeCase, inp=None):
    """The fp32 CPU truth's distance from the float64 one on the case's inputs, by the measures of the GPU test:
    (features max abs, d own rows worst prompt, d prefix per tensor); forward-only cases: features alone."""
    inp = inp or make_inputs(case)
    bw = case.route is not None
    r64, r32 = truth(case, inp, torch.float64, backward=bw), truth(case, inp, torch.float32, backward=bw)
    e_feat = float((r32["feats"].double() - r64["feats"]).abs().max())
    own = per_prompt_rel(r32["d_own"], r64["d_own"])[0] if bw else 0.0
    pfx = tensor_rel(r32["d_prefix"], r64["d_prefix"])[0] if bw and case.L > 0 else 0.0
    return e_feat, own, pfx, r64


if __name__ == "__main__":
    # how SEED_STEP was filled:  python tests/clip_shape_cases.py [case ...]
    found = {}
    for name in sys.argv[1:] or [c.name for c in CASES] + list(EXTRA):
        seen = []
        for step in range(12):
            SEED_STEP[name] = step
            e_feat, own, pfx, _ = yardstick(get(name))
            seen.append(max(e_feat, own, pfx))
            print(f"{name} step {step}: features {e_feat:.2e} d own/prompt {own:.2e} d prefix {pfx:.2e}", flush=True)
            if seen[-1] <= YARDSTICK_MAX:
                break
        found[name] = step if seen[-1] <= YARDSTICK_MAX else seen.index(min(seen))
        print(f"{name}: SEED_STEP {found[name]}" + ("" if seen[-1] <= YARDSTICK_MAX else f"  (none meets it: {min(seen):.2e})"), flush=True)
    print({k: v for k, v in found.items() if v})
