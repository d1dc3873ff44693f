"""Float64 truth of the CLIP text towers -- TEST INFRASTRUCTURE ONLY.

``clip_text_forward`` restates the reference's ``CLIPPromptEncoder.forward`` (model/prompt_encoder.py:64-92 over
model/clip/model.py:171-203: pre-LN blocks of nn.MultiheadAttention + QuickGELU MLP under the causal mask, the <eot> row pooled ->
ln_final -> text_projection) with plain torch ops on the FULL 77 positions, in whatever dtype its inputs have.  The reference itself
runs in fp32 only (its LayerNorm casts to fp32), so the tests' truth is this function in float64; tests/golden/make_golden_clip.py
pins it against the reference's fp32 run and stores the measured gap in every fixture (``gap_*``: fp32 rounding).
The HuggingFace tower has no fixture of its own: it is this function fed through the encoder's HF -> tower weight mapping
(``weights_from_slots``), which a CPU test checks against ``CLIPModel.get_text_features``."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import clip_text_cases as CC
from oracle import text_oracle as TO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-4


def load(name):
    return dict(np.load(os.path.join(GOLDEN, f"clip_{name}.npz")))


def clip_encoder(tower="small", seed=1):
    """this package's empty OpenAI-layout tower carrying the seeded weights (CPU)"""
    from vlsa_amd.prompt_encoder import CLIPPromptEncoder
    c = CC.TOWERS[tower]
    enc = CLIPPromptEncoder(width=c["width"], heads=c["heads"], layers=c["layers"], context_length=c["ctx"], vocab_size=c["vocab"],
                            output_dim=c["out_dim"])
    enc.load_state_dict(CC.make_clip_weights(tower, seed))
    return enc


def hf_model(tower="small", seed=1, hidden_act="quick_gelu", **text_kw):
    """a ``transformers`` CLIPModel (tiny vision side) whose text side carries the SAME seeded tensors under HuggingFace's names"""
    from transformers import CLIPConfig, CLIPModel, CLIPTextConfig, CLIPVisionConfig
    c = CC.TOWERS[tower]
    vision = CLIPVisionConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, image_size=32, patch_size=16)
    cfg = CLIPConfig(text_config=CLIPTextConfig(**dict(CC.hf_config_kwargs(tower, hidden_act), **text_kw)).to_dict(),
                     vision_config=vision.to_dict(), projection_dim=c["out_dim"])
    model = CLIPModel(cfg).eval()
    missing, unexpected = model.load_state_dict(CC.to_hf_state(CC.make_clip_weights(tower, seed), c["layers"]), strict=False)
    assert not unexpected and not [k for k in missing if k.startswith("text_")], (missing, unexpected)
    return model


def clip_text_forward(W, heads, prompts_embedding, pseudo_tokens, layers, act="quick_gelu", stats=None):
    """prompts_embedding [B, L, d] (L <= 77), pseudo_tokens [B, L] -> [B, out_dim]; W under OpenAI's names (clip_text_cases.py)"""
    B, L, d = prompts_embedding.shape
    mask = torch.full((L, L), float("-inf"), dtype=prompts_embedding.dtype).triu_(1)[None].expand(B, L, L)
    x = prompts_embedding + W["positional_embedding"][:L]
    for i in range(layers):
        p = f"transformer.resblocks.{i}."
        h = F.layer_norm(x, (d,), W[p + "ln_1.weight"], W[p + "ln_1.bias"], 1e-5)
        x = x + TO._mha(h, W[p + "attn.in_proj_weight"], W[p + "attn.in_proj_bias"], W[p + "attn.out_proj.weight"],
                        W[p + "attn.out_proj.bias"], heads, mask, stats)
        h = F.layer_norm(x, (d,), W[p + "ln_2.weight"], W[p + "ln_2.bias"], 1e-5)
        h = h @ W[p + "mlp.c_fc.weight"].t() + W[p + "mlp.c_fc.bias"]
        if stats is not None:
            stats["act_input_absmax"] = max(stats.get("act_input_absmax", 0.0), float(h.abs().max()))
        h = h * torch.sigmoid(1.702 * h) if act == "quick_gelu" else F.gelu(h)
        x = x + h @ W[p + "mlp.c_proj.weight"].t() + W[p + "mlp.c_proj.bias"]
    x = F.layer_norm(x, (d,), W["ln_final.weight"], W["ln_final.bias"], 1e-5)
    return x[torch.arange(B), pseudo_tokens.argmax(dim=-1)] @ W["text_projection"]


def eot_pseudo_tokens(text):
    """model/prompt_encoder.py:54-62 (the loop form)"""
    out = torch.zeros_like(text)
    for i, m in enumerate(text.argmax(dim=-1).tolist()):
        out[i, :m + 1] = torch.arange(1, m + 2)
    return out


def weights_from_slots(ts, token_embedding=None):
    """an encoder's ``_tower_tensors()`` (the slot order of vlsa_tt_model / vlsa_tt_layer) -> a weight dict under OpenAI's names"""
    W = {"positional_embedding": ts[0], "ln_final.weight": ts[2], "ln_final.bias": ts[3], "text_projection": ts[4]}
    names = ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias",
             "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias")
    for i in range((len(ts) - 5) // 12):
        for j, n in enumerate(names):
            W[f"transformer.resblocks.{i}.{n}"] = ts[5 + 12 * i + j]
    if token_embedding is not None:
        W["token_embedding.weight"] = token_embedding
    return {k: v.detach() for k, v in W.items()}


def f64(W, requires_grad=False):
    return {k: v.detach().double().clone().requires_grad_(requires_grad and k != "token_embedding.weight") for k, v in W.items()}


# ---- the rank cases: a RankPromptLearner in front of the tower ---------------------------------------------------------------------
def rank_case_inputs(case):
    (name, tower, seed, K, base, position) = case
    fx = load(name)
    table = {k[4:]: [int(v) for v in fx[k]] for k in fx if k.startswith("ids.")}
    c = CC.TOWERS[tower]
    return dict(W=CC.make_clip_weights(tower, seed), heads=c["heads"], layers=c["layers"], fx=fx, table=table,
                tok=CC.ReplayTokenizer(table, CC.BOS, CC.EOS, CC.PAD, length=CC.CTX), ctx_key="ctx",
                rank_keys=[f"rank{i}" for i in range(int(fx["rank_keys"]))], cfg=c)


def build_learner(case, inp):
    from vlsa_amd.prompt_learner import RankPromptLearner
    (name, tower, seed, K, base, position) = case
    E = torch.nn.Embedding.from_pretrained(inp["W"]["token_embedding.weight"].clone(), freeze=True)
    cfg = dict(max_num_tokens=CC.CTX, embedding_dim=E.embedding_dim, embedding_dtype=torch.float32)
    pl = RankPromptLearner(text_config=cfg, tokenizer=inp["tok"], token_embedding=E, num_base_ranks=base, num_ranks=K,
                           num_tokens_per_rank=4, num_context_tokens=8, rank_tokens_position=position,
                           init_context=inp["ctx_key"], init_rank_names=inp["rank_keys"])
    with torch.no_grad():
        pl.context_embeds.copy_(torch.from_numpy(inp["fx"]["context_embeds"]))
        pl.rank_embeds.copy_(torch.from_numpy(inp["fx"]["rank_embeds"]))
    return pl


def truth_rank_case(case, inp, W=None, act="quick_gelu", stats=None):
    """float64: sentences of the learner (oracle/text_oracle.py's restatement) through ``clip_text_forward``, then ``sum(feats * G)``
    backward.  Returns dict(features, context, rank, sentence, W) with the gradients on ``.grad`` of context / rank / W's tensors."""
    (name, tower, seed, K, base, position) = case
    fx = inp["fx"]
    W = f64(inp["W"], requires_grad=True) if W is None else W
    E = inp["W"]["token_embedding.weight"].double()
    ctx = torch.from_numpy(fx["context_embeds"]).double().requires_grad_(True)
    rk = torch.from_numpy(fx["rank_embeds"]).double().requires_grad_(True)
    pseudo = TO.pseudo_sentence_tokens(K, ctx.shape[0], rk.shape[1], max_tokens=CC.CTX)
    template = TO.sentence_template(E[CC.PAD], E[CC.BOS], E[CC.EOS], E[inp["table"]["X."][1]], pseudo)
    sent = TO.rank_prompt_learner_forward(ctx, rk, template, TO.interpolation_weights(base, K).double(), K, position)
    sent.retain_grad()
    feats = clip_text_forward(W, inp["heads"], sent, pseudo, inp["layers"], act, stats)
    (feats * torch.from_numpy(fx["G"]).double()).sum().backward()
    return dict(features=feats.detach(), context=ctx, rank=rk, sentence=sent, pseudo=pseudo, W=W)


_TRUTH = {}


def shared_truth(case):
    """the rank case's inputs and float64 truth, computed once per session and left unchanged"""
    if case[0] not in _TRUTH:
        inp = rank_case_inputs(case)
        stats = {}
        _TRUTH[case[0]] = (inp, truth_rank_case(case, inp, stats=stats), stats)
    return _TRUTH[case[0]]


def report(tag, what, got, want, rel):
    """print the figure, then return whether it holds: features within TOL (absolute); a gradient within TOL of its tensor's largest
    entry"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    bound = TOL * scale if rel else TOL
    print(f"[{tag}] {what}: max|err| {err:.3e} (max|truth| {scale:.3e}, bound {bound:.3e})")
    return err <= bound
