"""Sentence shapes at which the text tower (vlsa_amd/csrc/text_tower.hip) takes another path, and seeded inputs for them.

The rank-prompt fixtures hold every quantity the tower branches on at one or two values (K equal prompts of 12 or 13 compact rows, a
prefix of 4 or 5 positions).  The table below puts one case on each side of every threshold; tests/test_text_shape_cases_cpu.py pins
the (M, M_pad, max_len, prefix_len) column to ``compact_rows`` so that an edit cannot move a case off its boundary unnoticed, and
tests/test_gpu_text_tower_shapes.py runs every case against the float64 oracle.  Imports without a GPU.

A sentence of ``n`` non-pad pseudo tokens has ``n + 2`` rows (positions 0 .. n: the CLS token sees the first pad slot through the shifted
mask; plus the CLS row) -- except n = 127, a sentence without any pad: positions 0 .. 126 + a CLS row that attends to ITSELF (128 rows).

What the host code decides from a case's numbers (width 768, 12 heads):
    in_proj product     M <= 112: 16 x 64 tiles  k_tt_gemm<1, 4, 1, 12, 4> | <= 160: 32 x 48  <2, 4, 1, 12, 3> | else 48 x 48  <3, 4, 1, 12, 3>
    c_fc product        M <= 128: 16 x 96 tiles  k_tt_gemm<1, 4, 1, 12, 6> | <= 160: 32 x 64  <2, 4, 1, 12, 4> | else 48 x 48  <3, 4, 1, 12, 3>
    16-row products     M <= 160: 32-column tiles  <1, NW, 0, G, 2>        | else 48-column tiles  <1, NW, 0, G, 3>
    frozen backward     M <= 128: LayerNorm backward as a product prologue (k_tt_gemm<1, 4, 2, 12, ..>) | else one launch per stage
    M_pad               whole 96-row groups: 96 -> 96, 97 -> 192
    prefix keys         keys per key workgroup = the fewest kpb in 1 .. 4 with (K + 1 + ceil(L / kpb)) * heads <= 256, and only when
                        M <= 128; else the ticketed fold (``kpb`` 0 below).  12 heads, K = 12: 13 + ceil(L / kpb) <= 21, i.e.
                        L <= 8 -> 1, 9 .. 16 -> 2, 17 .. 24 -> 3, 25 .. 32 -> 4 (L = 25: groups of 4 keys, the 7th holds one), L >= 33 -> ticket.
                        The kernel's names do not show kpb; ``keys_per_workgroup`` restates the arithmetic and the CPU test holds the
                        column to it.
    attention           a wave per row of the longest prompt, 4 .. 16 waves: max_len > 16 makes the row loops run more than once;
                        the forward takes a second key chunk at S > 64; the backward and the persistent forward refuse max_len > 64.
"""
from __future__ import annotations

import zlib
from collections import namedtuple

import torch

import text_cases as TC

CTX = 128
# tower -> weight seed (all in TC.WEIGHT_SCALES at (3.5, 3.5): attention rows peaked, GELU inputs in the tails)
TOWER_SEEDS = {"w768x2": 9031, "w768x3": 9032, "w384x2": 9033, "w512x2": 9034, "w640x2": 9035, "small": 9036}

# name, tower, lens (non-pad pseudo tokens per prompt), L asked for; then what compact_rows must answer: M, M_pad, max_len, prefix_len;
# kpb: prefix keys per key workgroup of the attention backward (None: no prefix in the plan, 0: ticketed fold);
# route: the frozen tower's backward ("fused": PRO_LNBWD prologues, "stage": a launch per stage, None: forward only)
ShapeCase = namedtuple("ShapeCase", "name tower lens L M M_pad max_len prefix_len kpb route")


def _c(name, tower, lens, L, M, M_pad, max_len, prefix_len, kpb, route):
    return ShapeCase(name, tower, tuple(lens), L, M, M_pad, max_len, prefix_len, kpb, route)


CASES = [
    # ---- ragged prompts and the attention kernels' row loops (no prefix) ------------------------------------------------
    _c("ragged100", "w768x2", [1, 14, 15, 62], 0, 100, 192, 64, 0, None, "fused"),       # 3 .. 64 rows per prompt: 16 waves, 4 rounds
    _c("ragged154", "w768x2", [1, 2, 14, 15, 16, 30, 62], 0, 154, 192, 64, 0, None, "stage"),
    _c("one", "w768x2", [11], 0, 13, 96, 13, 0, None, "fused"),                          # a single prompt
    # ---- forward only: S = 64, 65, 128, 128 with the CLS row seeing itself, 3 --------------------------------------------
    _c("fwd_edges", "w768x2", [62, 63, 126, 127, 1], 0, 388, 480, 128, 0, None, None),
    # S = 66: the first length at which the second key chunk holds a key some row attends to (at S = 65 key 64 is the CLS row itself,
    # which only a sentence without a pad sees: there `S > 64` and `S > 65` compute the same)
    _c("fwd_S66", "w768x2", [64], 0, 66, 96, 66, 0, None, None),
    # ---- the row thresholds ---------------------------------------------------------------------------------------------
    _c("M96", "w768x2", [14] * 6, 0, 96, 96, 16, 0, None, "fused"),
    _c("M97", "w768x2", [14] * 5 + [15], 0, 97, 192, 17, 0, None, "fused"),
    _c("M112", "w768x2", [12] * 8, 0, 112, 192, 14, 0, None, "fused"),
    _c("M113", "w768x2", [12] * 7 + [13], 0, 113, 192, 15, 0, None, "fused"),
    _c("M128", "w768x2", [14] * 8, 0, 128, 192, 16, 0, None, "fused"),
    _c("M129", "w768x2", [14] * 7 + [15], 0, 129, 192, 17, 0, None, "stage"),
    _c("M160", "w768x2", [14] * 10, 0, 160, 192, 16, 0, None, "stage"),
    _c("M161", "w768x2", [14] * 9 + [15], 0, 161, 192, 17, 0, None, "stage"),
    # ---- shared prefix, K = 12: (K + 1 + ceil(L / kpb)) * 12 <= 256 ------------------------------------------------------
    _c("L8", "w768x2", [11] * 12, 8, 68, 96, 13, 8, 1, "fused"),              # 8 key workgroups per head
    _c("L9", "w768x2", [12] * 12, 9, 69, 96, 14, 9, 2, "fused"),              # 5 groups, the last holds one key
    _c("L17", "w768x2", [20] * 12, 17, 77, 96, 22, 17, 3, "fused"),           # 6 groups, the last holds two
    _c("L25", "w768x2", [28] * 12, 25, 85, 96, 30, 25, 4, "fused"),           # 7 groups, the last holds one
    _c("L33", "w768x2", [36] * 12, 33, 93, 96, 38, 33, 0, "fused"),           # no kpb <= 4 fits: ticket at M <= 128
    _c("L8M128", "w768x2", [16] * 12, 8, 128, 192, 18, 8, 1, "fused"),
    _c("L8M129", "w768x2", [16] * 11 + [17], 8, 129, 192, 19, 8, 0, "stage"),             # M > 128: ticket
    _c("S64pfx", "w768x2", [62, 62], 25, 103, 192, 64, 25, 2, "fused"),                   # (2 + 1 + 13) * 12 = 192; S = 64 with the prefix
    _c("K16L17", "w768x2", [18] * 16, 17, 65, 96, 20, 17, 0, "fused"),                    # (17 + 5) * 12 > 256 at kpb 4: ticket, 17 shares per key
    _c("raggedpfx", "w768x2", [9, 10, 14, 30, 9, 12], 9, 51, 96, 32, 9, 1, "fused"),      # (6 + 1 + 9) * 12 = 192; 0 .. 21 own tokens
    _c("fallback", "w768x2", [11] * 5 + [6], 8, 73, 96, 13, 0, None, "fused"),            # a prompt ends inside the prefix: planned with L = 0
    # ---- the other widths shape_of admits: runtime-G products, k_tt_ln_bwd (384, 640) / k_tt_ln_bwd4 with two slots (512) ----
    _c("w384_ragged100", "w384x2", [1, 14, 15, 62], 0, 100, 192, 64, 0, None, "stage"),
    _c("w384_L9", "w384x2", [12] * 12, 9, 69, 96, 14, 9, 1, "stage"),                     # 6 heads: (13 + 9) * 6 = 132
    _c("w512_ragged100", "w512x2", [1, 14, 15, 62], 0, 100, 192, 64, 0, None, "stage"),
    _c("w512_L9", "w512x2", [12] * 12, 9, 69, 96, 14, 9, 1, "stage"),                     # 8 heads: 22 * 8 = 176
    _c("w640_ragged100", "w640x2", [1, 14, 15, 62], 0, 100, 192, 64, 0, None, "stage"),
    _c("w640_L9", "w640x2", [12] * 12, 9, 69, 96, 14, 9, 1, "stage"),                     # 10 heads: 22 * 10 = 220
    # ---- three blocks: one that is neither top nor bottom ----------------------------------------------------------------
    _c("x3_L9", "w768x3", [12] * 12, 9, 69, 96, 14, 9, 2, "fused"),
]
BY_NAME = {c.name: c for c in CASES}

# cases outside the table above (refusals, their neighbours, the persistent forward's fall-backs): same columns
EXTRA = {c.name: c for c in [
    _c("S65", "w768x2", [63, 5], 0, 72, 96, 65, 0, None, None),                 # max_len 65: forward runs, backward refuses
    _c("ones22", "w768x2", [1] * 22, 0, 66, 96, 3, 0, None, "fused"),           # 22 x 12 = 264 attention workgroups
    _c("small_M1024", "small", [14] * 64, 0, 1024, 1056, 16, 0, None, "stage"),   # kPosRowsMax rows: the trainable tower's limit
    _c("small_M1040", "small", [11] * 80, 0, 1040, 1056, 13, 0, None, None),      # past it
]}
# what the trainable tower runs (every weight a leaf in the reference)
TRAIN_CASES = ["ragged100", "L9", "L25", "w384_ragged100", "w640_ragged100"]
# the cases the CPU test holds to the condition on the inputs (fp32 oracle within a quarter of the gate of the float64 one)
CONDITION_CASES = ["ragged100", "L9", "S64pfx"]
# The embeddings' seed is crc32(case name) + SEED_STEP[name].  The step is set by a rule that never looks at the GPU: the FIRST step in
# 0 .. 11 at which the fp32 CPU oracle stays within YARDSTICK_MAX of the float64 one by the GPU test's measures (features absolute, d own
# rows per prompt, d prefix per tensor), else the step in 0 .. 11 where that distance is smallest (`python tests/text_shape_cases.py`
# prints the search).  With in_proj / c_fc scaled by 3.5 the fp32 oracle's per-prompt distance is 1.3e-5 .. 3e-4 depending on the draw --
# the more prompts, the worse the worst of them -- and inputs on which plain fp32 misses the gate by itself say nothing about a kernel.
# No step in 0 .. 11 meets the condition for L33 (2.9e-5 at step 7), x3_L9 (3.2e-5 at step 1) and small_M1024 (64 prompts: 4.5e-5 at step 10).
SEED_STEP = {"ragged100": 1, "ragged154": 6, "one": 1, "M97": 1, "M112": 2, "M128": 2, "M129": 4, "M160": 8, "M161": 9,
             "L8": 1, "L9": 8, "L17": 1, "L25": 2, "L33": 7, "L8M128": 1, "L8M129": 5, "S64pfx": 1, "K16L17": 2, "fallback": 2,
             "w384_L9": 3, "w640_ragged100": 1, "w640_L9": 1, "x3_L9": 1, "ones22": 3, "small_M1024": 10}
GATE = 1e-4            # absolute on features; of the per-prompt (per-tensor) largest entry on gradients
YARDSTICK_MAX = 2.5e-5


def get(name) -> ShapeCase:
    return BY_NAME[name] if name in BY_NAME else EXTRA[name]


def keys_per_workgroup(case: ShapeCase):
    """The attention backward's choice for the prefix keys, restated from tt_backward: None without a prefix, 0 = ticketed fold."""
    if case.prefix_len == 0:
        return None
    heads, K, L = TC.TOWERS[case.tower]["heads"], len(case.lens), case.prefix_len
    if case.M <= 128 and heads <= 16:
        for kpb in (1, 2, 3, 4):
            if (K + 1 + -(-L // kpb)) * heads <= 256:
                return kpb
    return 0


def pseudo_tokens(lens) -> torch.Tensor:
    """[K, 127]: 1 .. n in front, zeros (pad) behind -- what the learners' ``pseudo_sentence_tokens`` hold."""
    out = torch.zeros(len(lens), CTX - 1, dtype=torch.long)
    for s, n in enumerate(lens):
        out[s, :n] = torch.arange(1, n + 1)
    return out


def make_weights(tower: str):
    return TC.make_tower_weights(tower, TOWER_SEEDS[tower])


def make_inputs(case: ShapeCase):
    """Seeded N(0, 0.02^2) embeddings (no learner in between): ``prefix`` [L, d] (None without one) and ``own`` [K, 127 - L, d], the two
    leaves of a shared-prefix case; ``pseudo`` [K, 127]; ``G`` [K, out_dim], the seeded weights of the scalar that is differentiated."""
    c = TC.TOWERS[case.tower]
    g = torch.Generator().manual_seed((zlib.crc32(case.name.encode()) + SEED_STEP.get(case.name, 0)) & 0x7FFFFFFF)
    K, d, L = len(case.lens), c["width"], case.L
    prefix = torch.randn(L, d, generator=g) * 0.02 if L > 0 else None
    own = torch.randn(K, CTX - 1 - L, d, generator=g) * 0.02
    G = torch.randn(K, c["out_dim"], generator=g)
    return dict(prefix=prefix, own=own, pseudo=pseudo_tokens(case.lens), G=G)


def assemble(prefix, own):
    """[K, 127, d] from the two leaves: autograd sums the prompts' shares of the prefix, as the kernel does."""
    if prefix is None:
        return own
    return torch.cat([prefix[None].expand(own.shape[0], *prefix.shape), own], dim=1)


def oracle(case: ShapeCase, inp, dtype=torch.float64, weight_grads=False, backward=True, W=None):
    """The CPU oracle over the full 128 positions in ``dtype``.  -> dict(feats, d_prefix, d_own, d_emb [K, 127, d], d_w {name: grad})."""
    from oracle import text_oracle as TO
    c = TC.TOWERS[case.tower]
    W = {k: v.to(dtype) for k, v in (W or make_weights(case.tower)).items()}
    if weight_grads:
        for k, v in W.items():
            v.requires_grad_(k != "token_embedding.weight")
    prefix = inp["prefix"].to(dtype).requires_grad_(backward) if inp["prefix"] is not None else None
    own = inp["own"].to(dtype).requires_grad_(backward)
    emb = assemble(prefix, own)
    with torch.set_grad_enabled(backward):
        feats = TO.prompt_encoder_forward(W, c["heads"], emb, inp["pseudo"], c["layers"])
    out = dict(feats=feats.detach(), d_prefix=None, d_own=None, d_emb=None, d_w=None)
    if backward:
        if prefix is not None:
            emb.retain_grad()
        (feats * inp["G"].to(dtype)).sum().backward()
        out.update(d_prefix=None if prefix is None else prefix.grad, d_own=own.grad, d_emb=emb.grad)
        if weight_grads:
            out["d_w"] = {k: v.grad for k, v in W.items() if k != "token_embedding.weight"}
    return out


def per_prompt_rel(got: torch.Tensor, ref: torch.Tensor):
    """max over prompts s of max|got_s - ref_s| / max|ref_s| (a 1-token prompt's large gradient cannot hide another prompt's error),
    with the worst prompt's absolute figures: (rel, abs err, max|ref_s|, s)."""
    got, ref = got.detach().to("cpu", torch.float64), ref.detach().to("cpu", torch.float64)
    worst = (0.0, 0.0, 0.0, -1)
    for s in range(ref.shape[0]):
        err, scale = float((got[s] - ref[s]).abs().max()), float(ref[s].abs().max())
        # (a prompt that ends inside the prefix has no own row in front of its first pad: reference exactly zero, and so must `got` be)
        rel = err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
        if rel >= worst[0]:
            worst = (rel, err, scale, s)
    return worst


def tensor_rel(got: torch.Tensor, ref: torch.Tensor):
    got, ref = got.detach().to("cpu", torch.float64), ref.detach().to("cpu", torch.float64)
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    return err / scale, err, scale


def yardstick(case: ShapeCase, inp=None):
    """The fp32 CPU oracle's distance from the float64 one on the case's inputs, by the measures of the GPU test:
    (features max abs, d own rows worst prompt, d prefix per tensor); forward-only cases: features alone."""
    inp = inp or make_inputs(case)
    bw = case.route is not None
    r64, r32 = oracle(case, inp, torch.float64, backward=bw), oracle(case, inp, torch.float32, backward=bw)
    e_feat = float((r32["feats"].double() - r64["feats"]).abs().max())
    own = per_prompt_rel(r32["d_own"], r64["d_own"])[0] if bw else 0.0
    pfx = tensor_rel(r32["d_prefix"], r64["d_prefix"])[0] if bw and case.L > 0 else 0.0
    return e_feat, own, pfx, r64


if __name__ == "__main__":
    # how SEED_STEP was filled:  python tests/text_shape_cases.py [case ...]
    import sys
    for name in sys.argv[1:] or [c.name for c in CASES] + [n for n in EXTRA if n != "small_M1040"]:
        seen = []
        for step in range(12):
            SEED_STEP[name] = step
            e_feat, own, pfx, _ = yardstick(get(name))
            seen.append(max(e_feat, own, pfx))
            print(f"{name} step {step}: features {e_feat:.2e} d own/prompt {own:.2e} d prefix {pfx:.2e}", flush=True)
            if seen[-1] <= YARDSTICK_MAX:
                break
        print(f"{name}: SEED_STEP {step if seen[-1] <= YARDSTICK_MAX else seen.index(min(seen))}", flush=True)
