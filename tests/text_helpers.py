"""Rebuild the inputs of a text-side golden case (tests/golden/text_*.npz) from seeds + the ids stored in the fixture."""
import os
import re
from collections import Counter

import numpy as np
import torch

import text_cases as TC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, f"text_{name}.npz")))


def table_of(fx):
    return {k[4:]: [int(v) for v in fx[k]] for k in fx if k.startswith("ids.")}


def rank_case_inputs(case):
    """-> dict(W, heads, layers, fx, table, tok, ctx_key, rank_keys, sizes) for a RANK_CASES entry."""
    (name, tower, seed, K, base, position) = case
    fx = load(name)
    W = TC.make_tower_weights(tower, seed)
    table = table_of(fx)
    bos, eos, pad = [int(v) for v in fx["special_ids"]]
    tok = TC.ReplayTokenizer(table, bos, eos, pad)
    rank_keys = [f"rank{i}" for i in range(int(fx["rank_keys"]))]
    c = TC.TOWERS[tower]
    return dict(W=W, heads=c["heads"], layers=c["layers"], fx=fx, table=table, tok=tok, ctx_key="ctx", rank_keys=rank_keys,
                special=(bos, eos, pad), cfg=c)


def oracle_rank_case(case, requires_grad=False):
    """Text features of a rank case through the CPU oracle.  Returns (features [K, out], leaves dict)."""
    from oracle import text_oracle as TO
    (name, tower, seed, K, base, position) = case
    inp = rank_case_inputs(case)
    fx, W, table = inp["fx"], inp["W"], inp["table"]
    bos, eos, pad = inp["special"]
    E = W["token_embedding.weight"]
    ctx = torch.from_numpy(fx["context_embeds"]).clone().requires_grad_(requires_grad)
    rk = torch.from_numpy(fx["rank_embeds"]).clone().requires_grad_(requires_grad)
    pseudo = TO.pseudo_sentence_tokens(K, ctx.shape[0], rk.shape[1])
    assert torch.equal(pseudo, torch.from_numpy(fx["pseudo"]))
    xdot = table["X."]
    template = TO.sentence_template(E[pad], E[bos], E[eos], E[xdot[1]], pseudo)
    interp = TO.interpolation_weights(base, K)
    assert np.abs(interp.numpy() - fx["interp"]).max() < 1e-6
    sent = TO.rank_prompt_learner_forward(ctx, rk, template, interp, K, position)
    feats = TO.prompt_encoder_forward(W, inp["heads"], sent, pseudo, inp["layers"])
    return feats, dict(context=ctx, rank=rk, sentence=sent, pseudo=pseudo)


def gemm_names(names):
    """Counter of the k_tt_gemm instantiations among the kernel names: 'MT, NW, PRO, G, NTW' -> launches"""
    return Counter(m.group(1) for n in names for m in [re.search(r"k_tt_gemm<([^>]*)>", n)] if m)


def expected_gemms_768(M, layers, route, act="gelu", out_dim=512):
    """What vlsa_tt_forward + vlsa_tt_backward launch for a frozen tower of width 768 (see the head comments of text_shape_cases.py and
    clip_shape_cases.py): template arguments <row tiles, waves, prologue (0 none, 1 LayerNorm, 2 LayerNorm backward; + 4 on the products
    with a GELU epilogue when ``act`` is "quick_gelu"), K groups, 16-column tiles>.  out_dim 512 or 768 (the d pooled product)."""
    q = {"gelu": 0, "quick_gelu": 4}[act]
    w = Counter()
    tw = 2 if M <= 160 else 3                                                      # the 16-row products' column tiles
    w["1, 4, 1, 12, 4" if M <= 112 else "2, 4, 1, 12, 3" if M <= 160 else "3, 4, 1, 12, 3"] += layers          # in_proj
    w[f"1, 4, {1 + q}, 12, 6" if M <= 128 else f"2, 4, {1 + q}, 12, 4" if M <= 160 else f"3, 4, {1 + q}, 12, 3"] += layers     # c_fc
    w[f"1, 4, 0, 12, {tw}"] += layers                                               # out_proj
    w[f"1, 8, 0, 24, {tw}"] += layers                                               # c_proj
    w["1, 4, 0, 12, 1"] += 1                                                        # text projection
    if route is None:
        return w
    w[{512: "1, 4, 0, 8, 1", 768: "3, 4, 0, 0, 2"}[out_dim]] += 1                   # d pooled (768: runtime K groups behind k_tt_tile_rows)
    w[f"1, 8, 0, 24, {tw}"] += layers                                               # d ln_2 out = d h_pre W_fc
    w[f"1, 8, 0, 18, {tw}"] += layers                                               # d ln_1 out = d qkv W_in
    if route == "fused":
        w[f"1, 4, {q}, 12, 6"] += 1                                                 # d h_pre, top block
        w[f"1, 4, {2 + q}, 12, 6"] += layers - 1                                    # ... below it: ln_1 backward of the block above as prologue
        w["1, 4, 2, 12, 2"] += layers                                               # d attn with ln_2 backward as prologue
    else:
        w[f"1, 4, {q}, 12, 6" if M <= 128 else f"2, 4, {q}, 12, 4" if M <= 160 else f"3, 4, {q}, 12, 3"] += layers      # d h_pre
        w[f"1, 4, 0, 12, {tw}"] += layers                                           # d attn
    return +w


def count(names, pattern):
    return sum(1 for n in names if re.search(pattern, n))


def tower_kernels(fn):
    """names of the HIP kernels `fn` launches (torch profiler, device activity only)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.key for e in prof.key_averages() for _ in range(e.count)]
