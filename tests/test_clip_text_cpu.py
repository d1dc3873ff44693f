"""Host side of the OpenAI-CLIP / HuggingFace-CLIP text towers on the CPU: construction and state-dict keys against the reference's
(tests/golden/clip_text_keys.json), the factory, the <eot>-pooled row plan, everything that is refused, the host-side validation of
``vlsa_tt_model.flags``, the float64 truth against the reference's fp32 fixtures, and the HF -> tower weight mapping against
``CLIPModel.get_text_features``."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import clip_text_cases as CC
import clip_text_helpers as CH

KEYS = json.load(open(os.path.join(CH.GOLDEN, "clip_text_keys.json")))


clip_encoder, hf_model = CH.clip_encoder, CH.hf_model


# ---- construction ---------------------------------------------------------------------------------------------------------------
def test_clip_encoder_has_the_references_keys_and_contract():
    enc = clip_encoder()
    assert {k: list(v.shape) for k, v in enc.state_dict().items()} == KEYS["CLIP"]
    assert enc.text_config == {"max_num_tokens": 77, "embedding_dim": 128, "embedding_dtype": torch.float32}
    assert enc.dtype == torch.float32 and enc.output_dim == 64 and enc.context_length == 77 and enc.cls_emb is None
    # adoption of a model object (what the loader hands over): the very same parameters, nothing copied
    from vlsa_amd.prompt_encoder import CLIPPromptEncoder
    adopted = CLIPPromptEncoder(enc)
    assert adopted.transformer is enc.transformer and adopted.text_projection is enc.text_projection
    assert list(adopted.state_dict()) == list(enc.state_dict()) and adopted.heads == 2


def test_clip_encoder_widens_fp16_weights_at_adoption():
    """the reference's loader hands fp16 weights (convert_weights): adoption widens them in place, exactly"""
    from vlsa_amd.prompt_encoder import CLIPPromptEncoder
    src = clip_encoder().half()
    want = {k: v.clone() for k, v in src.state_dict().items()}
    enc = CLIPPromptEncoder(src)
    assert all(p.dtype == torch.float32 for p in enc.parameters()) and enc.text_config["embedding_dtype"] == torch.float32
    for k, v in enc.state_dict().items():
        assert torch.equal(v, want[k].float()), k


def test_hf_encoder_keeps_huggingfaces_names():
    from vlsa_amd.prompt_encoder import HFCLIPPromptEncoder
    model = hf_model()
    enc = HFCLIPPromptEncoder(model)
    assert {k: list(v.shape) for k, v in enc.state_dict().items()} == KEYS["HF"]
    assert enc.encoder is model.text_model.encoder and enc.text_projection is model.text_projection
    assert enc.text_config == {"max_num_tokens": 77, "embedding_dim": 128, "embedding_dtype": torch.float32}
    assert enc.eos_token_id == CC.EOS and enc.output_dim == 64 and enc.heads == 2


def test_the_factory_builds_both_encoders():
    from vlsa_amd.model_utils import get_prompt_encoder
    from vlsa_amd.prompt_encoder import CLIPPromptEncoder, HFCLIPPromptEncoder, HipTextTower
    a, b = get_prompt_encoder(clip_encoder(), "CLIP"), get_prompt_encoder(hf_model(), "HF")
    assert type(a) is CLIPPromptEncoder and type(b) is HFCLIPPromptEncoder and isinstance(a, HipTextTower) and isinstance(b, HipTextTower)
    with pytest.raises(ValueError):
        get_prompt_encoder(None, "OpenCLIP")


def test_pseudo_tokens_follow_the_reference():
    rows = CC.token_rows([5, 75, 0, 30], 3)
    want = CH.eot_pseudo_tokens(rows)
    from vlsa_amd.prompt_encoder import HFCLIPPromptEncoder
    assert torch.equal(clip_encoder().generate_pseudo_tokens(rows), want)
    assert torch.equal(HFCLIPPromptEncoder(hf_model()).generate_pseudo_tokens(rows[:, :40]), CH.eot_pseudo_tokens(rows[:, :40]))
    assert want.argmax(dim=-1).tolist() == [6, 76, 1, 31]


# ---- the row plan ------------------------------------------------------------------------------------------------------------------
def pseudo_of(ms, L=77):
    out = torch.zeros(len(ms), L, dtype=torch.long)
    for i, m in enumerate(ms):
        out[i, :m + 1] = torch.arange(1, m + 2)
    return out


def test_plan_of_sot_eot_alone_is_two_rows():
    from vlsa_amd.prompt_encoder import last_token_rows
    rp = last_token_rows(pseudo_of([1]), 77)
    assert rp["row_pos"] == [0, 1] and rp["row_src"] == [0, 1] and rp["seq_row0"] == [0, 2] and rp["max_len"] == 2 and rp["M"] == 2
    assert rp["cls_keep"] == [1, 1] and rp["prefix_len"] == 0


def test_plan_reaches_the_last_position_and_mixes_lengths():
    from vlsa_amd.prompt_encoder import last_token_rows
    ms = [6, 76, 1, 31]
    rp = last_token_rows(pseudo_of(ms), 77)
    assert rp["M"] == sum(m + 1 for m in ms) and rp["max_len"] == 77 and rp["n_seq"] == 4
    assert rp["seq_row0"] == [0, 7, 84, 86, 118]
    for s, m in enumerate(ms):
        a, b = rp["seq_row0"][s], rp["seq_row0"][s + 1]
        assert rp["row_pos"][a:b] == list(range(m + 1)) and rp["row_seq"][a:b] == [s] * (m + 1)
        assert rp["row_pos"][b - 1] == m                               # the pooled row is the LAST row: the <eot> position
    assert rp["row_src"] == rp["row_pos"] and all(k == 1 for k in rp["cls_keep"]) and min(rp["row_src"]) >= 0
    # the pooled position is the ARGMAX of a row, whatever stands behind it
    odd = pseudo_of([4, 9])
    odd[0, 20] = 3
    assert last_token_rows(odd, 77)["seq_row0"] == [0, 5, 15]


def test_plan_shares_a_prefix_and_falls_back():
    from vlsa_amd.prompt_encoder import last_token_rows
    rp = last_token_rows(pseudo_of([10, 10, 12]), 77, prefix_len=5)
    assert rp["prefix_len"] == 5 and rp["row_pos"][:5] == [0, 1, 2, 3, 4] and rp["row_seq"][:5] == [0] * 5
    assert rp["seq_row0"] == [5, 11, 17, 25] and rp["M"] == 25 and rp["max_len"] == 13
    assert rp["row_pos"][5:11] == [5, 6, 7, 8, 9, 10] and rp["row_src"] == rp["row_pos"]
    # the pooled row may be the first row behind the prefix ...
    assert last_token_rows(pseudo_of([5, 8]), 77, prefix_len=5)["seq_row0"] == [5, 6, 10]
    # ... but a prompt that ends inside the prefix, or a single prompt, takes the plan without sharing
    for ms in ([4, 8], [9]):
        rp = last_token_rows(pseudo_of(ms), 77, prefix_len=5)
        assert rp["prefix_len"] == 0 and rp["seq_row0"][0] == 0 and rp["M"] == sum(m + 1 for m in ms)


def test_plan_takes_huggingfaces_shorter_rows_and_refuses_what_it_cannot_express():
    from vlsa_amd.prompt_encoder import last_token_rows
    rp = last_token_rows(pseudo_of([6, 39, 1], L=40), 77)
    assert rp["max_len"] == 40 and rp["seq_row0"] == [0, 7, 47, 49]
    with pytest.raises(ValueError, match="token positions"):
        last_token_rows(pseudo_of([3], L=78), 77)
    with pytest.raises(ValueError, match="<sot> and <eot>"):
        last_token_rows(torch.zeros(1, 77, dtype=torch.long), 77)
    gap = pseudo_of([8])
    gap[0, 3] = 0
    assert last_token_rows(gap, 77)["M"] == 9                          # OpenAI's tower masks no key: the zero means nothing
    with pytest.raises(NotImplementedError, match="zero in front of their maximum"):
        last_token_rows(gap, 77, refuse_gaps=True)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_unsupported_towers_are_refused_with_the_reason():
    from vlsa_amd._native import VlsaNativeError
    from vlsa_amd.prompt_encoder import CLIPPromptEncoder, CONCHPromptEncoder, HFCLIPPromptEncoder, QuickGELU
    src = clip_encoder()
    src.transformer.resblocks[1].mlp.gelu = nn.ReLU()
    with pytest.raises(NotImplementedError, match="activation ReLU"):
        CLIPPromptEncoder(src)
    src = clip_encoder()
    src.transformer.resblocks[0].ln_2.eps = 1e-6
    with pytest.raises(NotImplementedError, match="LayerNorm eps"):
        CLIPPromptEncoder(src)
    src = clip_encoder()
    src.transformer.resblocks[0].mlp.gelu = nn.GELU()                 # one erf block among QuickGELU blocks
    with pytest.raises(NotImplementedError, match="different activations"):
        CLIPPromptEncoder(src)
    for blk in src.transformer.resblocks:
        blk.mlp.gelu = nn.GELU()
    from vlsa_amd import _native as nat
    assert CLIPPromptEncoder(src)._tt_flags == nat.TT_POOL_LAST_TOKEN and CLIPPromptEncoder(clip_encoder())._tt_flags == 3
    assert isinstance(clip_encoder().transformer.resblocks[0].mlp.gelu, QuickGELU)
    # the CoCa tower still takes erf-GELU only
    from types import SimpleNamespace
    import text_cases as TC
    coca = CONCHPromptEncoder(width=128, heads=2, layers=2, vocab_size=64, output_dim=64)
    coca.load_state_dict(TC.make_tower_weights("small", 1))
    coca.transformer.resblocks[0].mlp.gelu = QuickGELU()
    with pytest.raises(NotImplementedError, match="activation QuickGELU"):
        CONCHPromptEncoder(SimpleNamespace(text=SimpleNamespace(pad_id=0, heads=2, **{k: getattr(coca, k) for k in (
            "positional_embedding", "transformer", "ln_final", "cls_emb", "text_projection", "token_embedding")})))
    # HuggingFace: activation, eps
    with pytest.raises(NotImplementedError, match="hidden_act 'gelu_new'"):
        HFCLIPPromptEncoder(hf_model(hidden_act="gelu_new"))
    with pytest.raises(NotImplementedError, match="LayerNorm eps"):
        HFCLIPPromptEncoder(hf_model(layer_norm_eps=1e-6))
    # ... a trainable tower under grad mode, CPU embeddings, a gap in the pseudo-tokens
    enc = HFCLIPPromptEncoder(hf_model())
    x, pt = torch.zeros(2, 77, 128), pseudo_of([5, 9])
    with pytest.raises(NotImplementedError, match="requires grad"):
        enc(prompts_embedding=x, prompts_pseudo_tokens=pt)
    for p in enc.parameters():
        p.requires_grad_(False)
    with pytest.raises(VlsaNativeError, match="CPU prompt embeddings"):
        enc(prompts_embedding=x, prompts_pseudo_tokens=pt)
    with pytest.raises(VlsaNativeError, match="CPU prompt embeddings"):
        clip_encoder()(prompts_embedding=x, prompts_pseudo_tokens=pt)
    pt[1, 2] = 0
    with pytest.raises(NotImplementedError, match="zero in front of their maximum"):
        enc._plan(pt, torch.device("cpu"))


def test_the_default_loaders_read_local_files_only(tmp_path):
    from vlsa_amd import hooks
    with pytest.raises(FileNotFoundError, match=os.path.join(str(tmp_path), "openai_clip", "ViT-B-16.pt")):
        hooks.load_vl_model({"name": "ViT-B/16"}, str(tmp_path), "CLIP")
    with pytest.raises(FileNotFoundError, match=os.path.join(str(tmp_path), "vinid/plip")):
        hooks.load_vl_model({"name": "vinid/plip"}, str(tmp_path), "HF")
    with pytest.raises(ValueError):
        hooks.load_vl_model({"name": "x"}, str(tmp_path), "OpenCLIP")
    # a state dict in OpenAI's layout (fp16, with the vision side and logit_scale next to the text side) -> the text side, fp32
    W = CC.make_clip_weights("small", 5)
    sd = {k: v.half() for k, v in W.items()}
    sd.update({"logit_scale": torch.tensor(2.5), "visual.proj": torch.zeros(4, 4).half(), "input_resolution": torch.tensor(32)})
    os.makedirs(tmp_path / "openai_clip")
    torch.save(sd, tmp_path / "openai_clip" / "ViT-B-16.pt")
    vl = hooks.load_vl_model({"name": "ViT-B/16"}, str(tmp_path), "CLIP")
    assert float(vl.logit_scale) == 2.5 and vl.heads == 2 and len(vl.transformer.resblocks) == 2
    from vlsa_amd.model_utils import get_prompt_encoder
    enc = get_prompt_encoder(vl, "CLIP")
    for k, v in enc.state_dict().items():
        assert v.dtype == torch.float32 and torch.equal(v, W[k].half().float()), k


def test_patch_reference_points_the_references_two_names_here(monkeypatch):
    import sys
    import types
    from vlsa_amd import prompt_encoder as pe
    from vlsa_amd.model_utils import patch_reference, unpatch_reference
    mods = {}
    for name in ("model", "model.utils", "model.vlsa", "model.deepmil", "model.prompt_encoder"):
        mods[name] = types.ModuleType(name)
        monkeypatch.setitem(sys.modules, name, mods[name])
        if "." in name:
            setattr(mods["model"], name.split(".")[1], mods[name])
    mods["model"].__path__ = []
    for mod, attrs in (("model.utils", ("VLSA",)), ("model.vlsa", ("VLSA", "logit_pooling")),
                       ("model.deepmil", ("VLFAN", "FeatMIL", "DeepMIL", "logit_pooling")),
                       ("model.prompt_encoder", ("CLIPPromptEncoder", "HFCLIPPromptEncoder", "CONCHPromptEncoder"))):
        for attr in attrs:
            setattr(mods[mod], attr, type(f"Original_{attr}", (), {}))
    ref_pe = mods["model.prompt_encoder"]
    originals = (ref_pe.CLIPPromptEncoder, ref_pe.HFCLIPPromptEncoder, ref_pe.CONCHPromptEncoder)
    saved = patch_reference()
    try:
        assert ref_pe.CLIPPromptEncoder is pe.CLIPPromptEncoder and ref_pe.HFCLIPPromptEncoder is pe.HFCLIPPromptEncoder
        assert ref_pe.CONCHPromptEncoder is originals[2]
    finally:
        unpatch_reference(saved)
    assert (ref_pe.CLIPPromptEncoder, ref_pe.HFCLIPPromptEncoder, ref_pe.CONCHPromptEncoder) == originals


# ---- the C ABI's host-side validation ---------------------------------------------------------------------------------------------
def test_bad_flags_and_a_missing_cls_embedding_are_einval_on_the_host():
    """nothing is launched: every call below returns from the validation in front of the first kernel"""
    from vlsa_amd import _native as nat
    lib = nat.load()
    TTLayer, TTModel, TTRows = (nat.STRUCTS[n] for n in ("vlsa_tt_layer", "vlsa_tt_model", "vlsa_tt_rows"))
    assert TTModel._fields_[-1][0] == "flags" and (nat.TT_ACT_QUICK_GELU, nat.TT_POOL_LAST_TOKEN) == (1, 2) and nat.ABI_VERSION == 1
    layers = (TTLayer * 2)()
    buf = ctypes.create_string_buffer(64)                              # stands in for every pointer: never dereferenced
    p = ctypes.addressof(buf)
    rows = TTRows(2, 10, 96, 6, p, p, p, p, p, 0)

    def model(cls, flags):
        return TTModel(128, 2, 2, 64, 77, layers, p, cls, p, p, p, flags)

    def calls(m):
        return (lib.vlsa_tt_packed_bytes(ctypes.byref(m), 1), lib.vlsa_tt_workspace_bytes(ctypes.byref(m), ctypes.byref(rows), 1),
                lib.vlsa_tt_pack_weights(ctypes.byref(m), p, 1, None),
                lib.vlsa_tt_forward(ctypes.byref(m), ctypes.byref(rows), p, p, 77 * 128, 128, p, 0, p, None),
                lib.vlsa_tt_backward(ctypes.byref(m), ctypes.byref(rows), p, p, p, p, 77 * 128, 128, 2 * 77 * 128, None))
    for bad in (model(p, 4), model(p, 7), model(p, -1), model(None, 0), model(None, nat.TT_ACT_QUICK_GELU)):
        assert calls(bad) == (0, 0, nat.EINVAL, nat.EINVAL, nat.EINVAL)
    # accepted (sizes only: the launching calls are for the GPU tests); flagged models never take the persistent forward
    for ok in (model(p, 0), model(p, 1), model(None, 2), model(None, 3), model(p, 3)):
        assert lib.vlsa_tt_packed_bytes(ctypes.byref(ok), 1) > 0 and lib.vlsa_tt_workspace_bytes(ctypes.byref(ok), ctypes.byref(rows), 1) > 0
    wide = (TTLayer * 12)()
    for flags in (1, 2, 3):
        m = TTModel(768, 12, 12, 512, 77, wide, p, p, p, p, p, flags)
        assert lib.vlsa_tt_status_offset(ctypes.byref(m), ctypes.byref(rows), nat.TT_PERSISTENT) == -1
    m = TTModel(768, 12, 12, 512, 128, wide, p, p, p, p, p, 0)
    assert lib.vlsa_tt_status_offset(ctypes.byref(m), ctypes.byref(rows), nat.TT_PERSISTENT) >= 0


# ---- truth ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CC.RANK_CASES, ids=[c[0] for c in CC.RANK_CASES])
def test_the_float64_truth_is_the_references_fp32_run_up_to_rounding(case):
    """the fixture holds the REFERENCE's features and gradients (fp32) and the gap the recipe measured against the float64 restatement;
    the restatement run here lands on the same gap (the bound is make_golden_clip.GAP_BOUND: half the GPU tests' gate)"""
    inp, truth, stats = CH.shared_truth(case)
    fx = inp["fx"]
    pl = CH.build_learner(case, inp)
    assert torch.equal(pl.pseudo_sentence_tokens, torch.from_numpy(fx["pseudo"])) and pl.pseudo_sentence_tokens.shape[1] == 77
    s = pl().detach().double()
    assert np.allclose([float(s.sum()), float((s ** 2).sum())], fx["sentence_checksum"], rtol=1e-6)
    assert (s - truth["sentence"].detach()).abs().max().item() < 1e-6
    for what, got, ref, gap in (("features", truth["features"], fx["text_features"], fx["gap_features"]),
                                ("grad_context", truth["context"].grad, fx["grad_context"], fx["gap_grad_context"]),
                                ("grad_rank", truth["rank"].grad, fx["grad_rank"], fx["gap_grad_rank"])):
        err, scale = np.abs(got.numpy() - ref).max(), 1.0 if what == "features" else np.abs(ref).max()
        print(f"[{case[0]}] {what}: truth vs reference fp32 {err:.2e} (recorded {float(gap):.2e}, max|ref| {np.abs(ref).max():.2e})")
        assert abs(err - float(gap)) <= 1e-9 * max(1.0, np.abs(ref).max()) and err < 5e-5 * scale
    print(f"[{case[0]}] largest activation input {stats['act_input_absmax']:.2f}, largest attention logit {stats['attn_logit_absmax']:.2f}")
    if case[2] in CC.WEIGHT_SCALES:
        assert stats["act_input_absmax"] > 6.0


@pytest.mark.parametrize("case", CC.TEXT_CASES, ids=[c[0] for c in CC.TEXT_CASES])
def test_the_truth_on_tokenised_text(case):
    (name, tower, seed, lens) = case
    fx, c = CH.load(name), CC.TOWERS[tower]
    rows = torch.from_numpy(fx["token_ids"])
    assert torch.equal(rows, CC.token_rows(lens, seed + 2))
    W = CH.f64(CC.make_clip_weights(tower, seed))
    truth = CH.clip_text_forward(W, c["heads"], W["token_embedding.weight"][rows], CH.eot_pseudo_tokens(rows), c["layers"])
    err = np.abs(truth.numpy() - fx["text_features"]).max()
    print(f"[{name}] truth vs reference fp32 {err:.2e} (recorded {float(fx['gap_features']):.2e})")
    assert abs(err - float(fx["gap_features"])) <= 1e-9 and err < 5e-5


@pytest.mark.parametrize("hidden_act", ["quick_gelu", "gelu"])
def test_the_hf_weight_mapping_against_huggingfaces_own_text_path(hidden_act):
    """HF truth = the float64 restatement fed through the ENCODER'S OWN HF -> tower mapping (``_tower_tensors``): checked here against
    ``CLIPModel.get_text_features`` on a seeded tiny config with eos_token_id != 2 (id 2 takes HuggingFace's legacy argmax branch).
    Rows shorter than 77, as HuggingFace's tokenizer pads."""
    from vlsa_amd.prompt_encoder import HFCLIPPromptEncoder
    model = hf_model("small", 7, hidden_act)
    assert model.config.text_config.eos_token_id == CC.EOS != 2
    enc = HFCLIPPromptEncoder(model)
    ts = enc._tower_tensors()
    assert ts[1] is None and ts[4].shape == (128, 64) and ts[7].shape == (384, 128) and ts[8].shape == (384,) and len(ts) == 5 + 12 * 2
    W = CH.f64(CH.weights_from_slots(ts, enc.token_embedding.weight))
    rows = CC.token_rows([5, 38, 0, 30], 11, length=40)
    with torch.no_grad():
        theirs = model.get_text_features(input_ids=rows, attention_mask=(rows != CC.PAD).long())
    theirs = getattr(theirs, "pooler_output", theirs)
    pseudo = enc.generate_pseudo_tokens(rows)
    ours = CH.clip_text_forward(W, enc.heads, W["token_embedding.weight"][rows], pseudo, 2, act=hidden_act)
    err = (ours - theirs.double()).abs().max().item()
    print(f"[hf mapping, {hidden_act}] float64 truth through the encoder's mapping vs CLIPModel.get_text_features (fp32): {err:.2e}")
    assert err < 5e-5
    # the derived operands follow their sources: in place (same storage, version bumped), and only when a source changed
    in_w, proj = ts[7], ts[4]
    assert enc._tower_tensors() is ts
    with torch.no_grad():
        model.text_model.encoder.layers[0].self_attn.k_proj.weight.mul_(2.0)
        model.text_projection.weight.add_(1.0)
    v0 = in_w._version
    ts2 = enc._tower_tensors()
    assert ts2[7] is in_w and ts2[7].data_ptr() == in_w.data_ptr() and in_w._version > v0 and ts2[4] is proj
    assert torch.equal(in_w[128:256], model.text_model.encoder.layers[0].self_attn.k_proj.weight)
    assert torch.equal(proj, model.text_projection.weight.t())
