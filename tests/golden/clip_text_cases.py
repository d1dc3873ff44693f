"""Seeded CLIP-text-tower weights and inputs for the fixtures of the OpenAI-CLIP / HuggingFace-CLIP towers (tests/golden/clip_*.npz,
made by tests/golden/make_golden_clip.py).  As in text_cases.py every tensor is regenerated from a seed (the same torch CPU generator
wherever the tests run); names follow the state dict of the reference's ``CLIPPromptEncoder`` (model/prompt_encoder.py:39-47 over
model/clip/model.py:171-203,285-297), and ``to_hf_state`` renames the same tensors into a ``transformers`` ``CLIPModel``."""
from __future__ import annotations

import torch

from text_cases import ReplayTokenizer, synthetic_prompt_table  # noqa: F401  (re-exported: the learners of the rank cases use them)

CTX = 77
# ids of the made-up vocabulary (64 tokens): OpenAI's tokenizer gives <eot> the HIGHEST id of a sentence (the encoder pools the argmax
# row), so <sot> / <eot> sit at the top, ordinary tokens are 3 .. 61, pad is 0
VOCAB, BOS, EOS, PAD = 64, 62, 63, 0
TOWERS = {
    "small": dict(width=128, heads=2, layers=2, vocab=VOCAB, ctx=CTX, out_dim=64),
    "w512x2": dict(width=512, heads=8, layers=2, vocab=VOCAB, ctx=CTX, out_dim=512),    # the ViT-B text tower at a sixth of the weights
    "w128x3": dict(width=128, heads=2, layers=3, vocab=VOCAB, ctx=CTX, out_dim=64),     # a block that is neither first nor last
    # width 768 / 12 heads: the products' static-G shapes (tests/clip_shape_cases.py)
    "w768x2": dict(width=768, heads=12, layers=2, vocab=VOCAB, ctx=CTX, out_dim=512),
    "w768x3": dict(width=768, heads=12, layers=3, vocab=VOCAB, ctx=CTX, out_dim=512),
    "w768x2_o768": dict(width=768, heads=12, layers=2, vocab=VOCAB, ctx=CTX, out_dim=768),   # the ViT-L/14 text side's projection
}
# as text_cases.WEIGHT_SCALES: in_proj / c_fc weights rescaled after the draw, so that the attention logits and the QuickGELU inputs
# leave the range of a freshly initialised tower (|x| past 6: the sigmoid's tails).  seed -> (in_proj factor, c_fc factor)
WEIGHT_SCALES = {9121: (3.5, 3.5),
                 9141: (3.5, 3.5), 9142: (3.5, 3.5), 9143: (3.5, 3.5)}     # the 768-wide towers of tests/clip_shape_cases.py


def make_clip_weights(name: str, seed: int):
    """N(0, std) with the stds of CLIP.initialize_parameters (model/clip/model.py:299-326); biases and LayerNorm affine parameters
    non-trivial so that they are exercised.  No ``cls_emb``: the tower has no CLS token."""
    c = TOWERS[name]
    d, L = c["width"], c["layers"]
    g = torch.Generator().manual_seed(seed)
    n = lambda *s, std: torch.randn(*s, generator=g) * std   # noqa: E731
    proj_std, attn_std, fc_std = (d ** -0.5) * ((2 * L) ** -0.5), d ** -0.5, (2 * d) ** -0.5
    W = {"token_embedding.weight": n(c["vocab"], d, std=0.02), "positional_embedding": n(c["ctx"], d, std=0.01),
         "text_projection": n(d, c["out_dim"], std=d ** -0.5), "ln_final.weight": 1 + n(d, std=0.1), "ln_final.bias": n(d, std=0.05)}
    for i in range(L):
        p = f"transformer.resblocks.{i}."
        W[p + "ln_1.weight"], W[p + "ln_1.bias"] = 1 + n(d, std=0.1), n(d, std=0.05)
        W[p + "attn.in_proj_weight"], W[p + "attn.in_proj_bias"] = n(3 * d, d, std=attn_std), n(3 * d, std=0.02)
        W[p + "attn.out_proj.weight"], W[p + "attn.out_proj.bias"] = n(d, d, std=proj_std), n(d, std=0.02)
        W[p + "ln_2.weight"], W[p + "ln_2.bias"] = 1 + n(d, std=0.1), n(d, std=0.05)
        W[p + "mlp.c_fc.weight"], W[p + "mlp.c_fc.bias"] = n(4 * d, d, std=fc_std), n(4 * d, std=0.02)
        W[p + "mlp.c_proj.weight"], W[p + "mlp.c_proj.bias"] = n(d, 4 * d, std=proj_std), n(d, std=0.02)
    if seed in WEIGHT_SCALES:
        s_in, s_fc = WEIGHT_SCALES[seed]
        for i in range(L):
            p = f"transformer.resblocks.{i}."
            W[p + "attn.in_proj_weight"] = W[p + "attn.in_proj_weight"] * s_in
            W[p + "mlp.c_fc.weight"] = W[p + "mlp.c_fc.weight"] * s_fc
    return W


def to_hf_state(W: dict, layers: int) -> dict:
    """the same tensors under the names of ``CLIPModel.text_model`` / ``CLIPModel.text_projection``: q / k / v are the thirds of the
    in-projection, ``text_projection.weight`` is [out, width] (the transpose)"""
    H = {"text_model.embeddings.token_embedding.weight": W["token_embedding.weight"],
         "text_model.embeddings.position_embedding.weight": W["positional_embedding"],
         "text_model.final_layer_norm.weight": W["ln_final.weight"], "text_model.final_layer_norm.bias": W["ln_final.bias"],
         "text_projection.weight": W["text_projection"].t().contiguous()}
    for i in range(layers):
        p, h = f"transformer.resblocks.{i}.", f"text_model.encoder.layers.{i}."
        d = W[p + "ln_1.weight"].shape[0]
        for j, name in enumerate("qkv"):
            H[h + f"self_attn.{name}_proj.weight"] = W[p + "attn.in_proj_weight"][j * d:(j + 1) * d].clone()
            H[h + f"self_attn.{name}_proj.bias"] = W[p + "attn.in_proj_bias"][j * d:(j + 1) * d].clone()
        for ours, theirs in (("attn.out_proj", "self_attn.out_proj"), ("ln_1", "layer_norm1"), ("ln_2", "layer_norm2"),
                             ("mlp.c_fc", "mlp.fc1"), ("mlp.c_proj", "mlp.fc2")):
            H[h + theirs + ".weight"], H[h + theirs + ".bias"] = W[p + ours + ".weight"], W[p + ours + ".bias"]
    return H


def hf_config_kwargs(name: str, hidden_act: str = "quick_gelu") -> dict:
    """``CLIPTextConfig`` arguments of a tower (``eos_token_id`` is NOT 2: id 2 takes HuggingFace's legacy argmax pooling branch)"""
    c = TOWERS[name]
    return dict(vocab_size=c["vocab"], hidden_size=c["width"], intermediate_size=4 * c["width"], projection_dim=c["out_dim"],
                num_hidden_layers=c["layers"], num_attention_heads=c["heads"], max_position_embeddings=c["ctx"], hidden_act=hidden_act,
                layer_norm_eps=1e-5, attention_dropout=0.0, pad_token_id=PAD, bos_token_id=BOS, eos_token_id=EOS)


def token_rows(lens, seed: int, length: int = CTX) -> torch.Tensor:
    """[len(lens), length] ids: <sot>, n ordinary tokens, <eot>, pads"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.full((len(lens), length), PAD, dtype=torch.long)
    for i, n in enumerate(lens):
        rows[i, 0] = BOS
        rows[i, 1:1 + n] = torch.randint(3, BOS, (n,), generator=g)
        rows[i, 1 + n] = EOS
    return rows


def prompt_table(seed: int, base: int):
    """made-up context + rank names (ordinary ids only), as make_golden_text.py draws them for the CoCa cases"""
    return synthetic_prompt_table(BOS, seed, n_ctx=3 if base == 3 else 4, rank_lens=(4, 3, 3, 4)[:base] if base != 3 else (2, 4, 3))


# ---- fixture cases -------------------------------------------------------------------------------------------
# a RankPromptLearner through the tower: name, tower, weight seed, num_ranks (K), num_base_ranks, rank_tokens_position
RANK_CASES = [
    ("rank_small_k8_front", "small", 9101, 8, 4, "front"),
    ("rank_w512_k12_tail", "w512x2", 9102, 12, 4, "tail"),
    ("rank_l3_k5_middle", "w128x3", 9103, 5, 3, "middle"),
    ("rank_w512_k12_hot", "w512x2", 9121, 12, 4, "tail"),          # rescaled weights (WEIGHT_SCALES)
]
# tokenised texts: name, tower, weight seed, sentence lengths (tokens between <sot> and <eot>).  75 puts <eot> on the last position
# (76) and needs the attention's second key chunk, 0 is <sot><eot> alone (two rows)
TEXT_CASES = [
    ("text_small", "small", 9111, [5, 75, 0, 30]),
    ("text_w512", "w512x2", 9112, [5, 75, 0, 30]),
    ("text_l3", "w128x3", 9113, [5, 75, 0, 30]),
]
