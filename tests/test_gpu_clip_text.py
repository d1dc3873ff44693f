"""The OpenAI-CLIP and HuggingFace-CLIP text towers on the GPU (``CLIPPromptEncoder`` / ``HFCLIPPromptEncoder``: QuickGELU, the <eot> row
pooled) against the float64 truth of tests/clip_text_helpers.py, which tests/test_clip_text_cpu.py pins to the reference's fp32 run.
Gates are the text side's existing ones: features within 1e-4, every gradient within 1e-4 of its tensor's largest entry; every
comparison prints its figure first (``CH.report``)."""
import os

import pytest
import torch

import cases
import clip_text_cases as CC
import clip_text_helpers as CH

pytestmark = pytest.mark.gpu
HOT = [c for c in CC.RANK_CASES if c[2] in CC.WEIGHT_SCALES]


def clip_on_gpu(tower, seed, trainable=False):
    enc = CH.clip_encoder(tower, seed)
    for k, p in enc.named_parameters():
        p.requires_grad_(trainable and k != "token_embedding.weight")
    return enc.cuda().eval()


def hf_on_gpu(tower, seed, hidden_act="quick_gelu"):
    from vlsa_amd.prompt_encoder import HFCLIPPromptEncoder
    enc = HFCLIPPromptEncoder(CH.hf_model(tower, seed, hidden_act))
    for p in enc.parameters():
        p.requires_grad_(False)
    return enc.cuda().eval()


def text_truth(tower, seed, rows, act="quick_gelu"):
    c = CC.TOWERS[tower]
    W = CH.f64(CC.make_clip_weights(tower, seed))
    return CH.clip_text_forward(W, c["heads"], W["token_embedding.weight"][rows], CH.eot_pseudo_tokens(rows), c["layers"], act)


# ---- 1. tokenised text: the 2-row prompt, the last position, the attention's second key chunk ----------------------------------------
@pytest.mark.parametrize("case", CC.TEXT_CASES, ids=[c[0] for c in CC.TEXT_CASES])
def test_tokenised_text_forward(case):
    (name, tower, seed, lens) = case
    assert lens == [5, 75, 0, 30]
    rows = torch.from_numpy(CH.load(name)["token_ids"])
    enc = clip_on_gpu(tower, seed)
    with torch.no_grad():
        feats = enc(prompts_text=rows.cuda())
        plan = enc._plan(enc.generate_pseudo_tokens(rows), feats.device)
        assert (plan.M, plan.max_len, plan.prefix_len) == (7 + 77 + 2 + 32, 77, 0)
        assert CH.report(name, "features (prompts_text)", feats, text_truth(tower, seed, rows), rel=False)
        # rows behind <eot> are never read: not even NaNs get through; the <eot> slot itself is read
        emb = enc.token_embedding(rows.cuda())
        pseudo = enc.generate_pseudo_tokens(rows.cuda())
        junk = emb.clone()
        for i, m in enumerate(pseudo.argmax(dim=-1).tolist()):
            junk[i, m + 1:] = float("nan")
        assert torch.equal(enc(prompts_embedding=junk, prompts_pseudo_tokens=pseudo), feats)
        junk = emb.clone()
        junk[2, 1] += 0.3 * torch.randn(junk.shape[2], generator=torch.Generator().manual_seed(2)).cuda()     # (not a constant: LayerNorm removes one)
        assert (enc(prompts_embedding=junk, prompts_pseudo_tokens=pseudo)[2] - feats[2]).abs().max().item() > 1e-3


# ---- 2. + 3. rank prompts through the frozen tower, shared prefix on and off; rescaled weights ----------------------------------------
def check_sentence_gradient(tag, got, truth, L, ms):
    """d prompts_embedding [K, 77, d].  With a shared prefix of L positions the prefix rows are planned once, as prompt 0's: their
    gradient -- the sum over the prompts -- lands in prompt 0 and the other prompts' prefix slots get zeros."""
    want = truth.clone()
    if L > 0:
        want[0, :L] = truth[:, :L].sum(0)
        want[1:, :L] = 0
    ok = CH.report(tag, "d prompts_embedding", got, want, rel=True)
    eot = torch.stack([got[i, m] for i, m in enumerate(ms)]).cpu().double()
    eot_want = torch.stack([want[i, m] for i, m in enumerate(ms)])
    scale = want.abs().max().item()
    err = (eot - eot_want).abs().max().item()
    print(f"[{tag}] d prompts_embedding on the <eot> slots: max|err| {err:.3e}, max|truth there| {eot_want.abs().max().item():.3e}")
    assert eot_want.abs().max().item() > 1e-3 * scale and err <= CH.TOL * scale        # the pooled row's gradient is a token gradient
    for i, m in enumerate(ms):
        assert float(got[i, m + 1:].abs().max()) == 0.0                                # nothing behind <eot>
    return ok


@pytest.mark.parametrize("prefix", [False, True], ids=["rows", "shared_prefix"])
@pytest.mark.parametrize("case", CC.RANK_CASES, ids=[c[0] for c in CC.RANK_CASES])
def test_rank_prompts_through_the_frozen_tower(case, prefix):
    (name, tower, seed, K, base, position) = case
    inp, truth, stats = CH.shared_truth(case)
    tag = f"{name}, {'shared prefix' if prefix else 'rows'}"
    print(f"[{tag}] largest activation input {stats['act_input_absmax']:.2f}, largest attention logit {stats['attn_logit_absmax']:.2f}")
    if case in HOT:
        assert stats["act_input_absmax"] > 6.0
    enc = clip_on_gpu(tower, seed)
    pl = CH.build_learner(case, inp).cuda()
    L = pl.shared_prefix_len if prefix else 0
    tok = pl.pseudo_sentence_tokens
    ms = tok.argmax(dim=-1).tolist()
    with torch.no_grad():
        f0 = enc(prompts_embedding=pl(), prompts_pseudo_tokens=tok, shared_prefix_len=L)          # inference route (nothing saved)
    plan = enc._plan(tok, f0.device, L)
    assert plan.prefix_len == L and plan.M == K * (ms[0] + 1) - (K - 1) * L
    if prefix:
        assert L == (1 if position == "front" else 1 + (pl.context_embeds.shape[0] // 2 if position == "middle" else pl.context_embeds.shape[0]))
    ok = CH.report(tag, "features (no grad)", f0, truth["features"], rel=False)
    sent = pl()
    sent.retain_grad()
    feats = enc(prompts_embedding=sent, prompts_pseudo_tokens=tok, shared_prefix_len=L)
    assert type(feats.grad_fn).__name__ == "_TextTowerFnBackward" and torch.equal(feats.detach(), f0)
    (feats * torch.from_numpy(inp["fx"]["G"]).cuda()).sum().backward()
    ok &= check_sentence_gradient(tag, sent.grad, truth["sentence"].grad, L, ms)
    ok &= CH.report(tag, "d context_embeds", pl.context_embeds.grad, truth["context"].grad, rel=True)
    ok &= CH.report(tag, "d rank_embeds", pl.rank_embeds.grad, truth["rank"].grad, rel=True)
    assert ok


# ---- 4. the trainable tower: every parameter's gradient -------------------------------------------------------------------------------
@pytest.mark.parametrize("case,prefix", [(CC.RANK_CASES[0], False), (CC.RANK_CASES[0], True), (CC.RANK_CASES[1], True), (CC.RANK_CASES[2], False)],
                         ids=lambda v: v[0] if isinstance(v, tuple) else ("shared_prefix" if v else "rows"))
def test_trainable_clip_tower_weight_gradients(case, prefix):
    (name, tower, seed, K, base, position) = case
    inp, truth, _ = CH.shared_truth(case)
    tag = f"trainable {name}, {'shared prefix' if prefix else 'rows'}"
    enc = clip_on_gpu(tower, seed, trainable=True)
    pl = CH.build_learner(case, inp).cuda()
    feats = enc(prompts_embedding=pl(), prompts_pseudo_tokens=pl.pseudo_sentence_tokens, shared_prefix_len=pl.shared_prefix_len if prefix else 0)
    assert type(feats.grad_fn).__name__ == "_TextTowerTrainFnBackward"
    ok = CH.report(tag, "features", feats, truth["features"], rel=False)
    (feats * torch.from_numpy(inp["fx"]["G"]).cuda()).sum().backward()
    ok &= CH.report(tag, "d context_embeds", pl.context_embeds.grad, truth["context"].grad, rel=True)
    ok &= CH.report(tag, "d rank_embeds", pl.rank_embeds.grad, truth["rank"].grad, rel=True)
    params, checked = dict(enc.named_parameters()), 0
    assert "cls_emb" not in params
    for k, w in truth["W"].items():
        if k == "token_embedding.weight":
            continue
        assert params[k].grad is not None, k
        ok &= CH.report(tag, "d " + k, params[k].grad, w.grad, rel=True)
        cases.record_grad_error(tag + ": " + k, (params[k].grad.cpu().double() - w.grad).abs().max().item(), w.grad.abs().max().item(),
                                CH.TOL * w.grad.abs().max().item())
        checked += 1
    assert checked == 4 + 12 * inp["layers"] and params["token_embedding.weight"].grad is None
    assert ok


# ---- 5. HuggingFace layout: the same kernels on the same operands ---------------------------------------------------------------------
@pytest.mark.parametrize("case", CC.RANK_CASES[:2], ids=[c[0] for c in CC.RANK_CASES[:2]])
def test_hf_layout_is_bit_equal_to_the_clip_layout(case):
    (name, tower, seed, K, base, position) = case
    inp, truth, _ = CH.shared_truth(case)
    G = torch.from_numpy(inp["fx"]["G"]).cuda()
    out = {}
    for layout, enc in (("clip", clip_on_gpu(tower, seed)), ("hf", hf_on_gpu(tower, seed))):
        pl = CH.build_learner(case, inp).cuda()
        sent = pl()
        sent.retain_grad()
        feats = enc(prompts_embedding=sent, prompts_pseudo_tokens=pl.pseudo_sentence_tokens, shared_prefix_len=pl.shared_prefix_len)
        (feats * G).sum().backward()
        out[layout] = (feats.detach().clone(), sent.grad.clone())
        assert enc._c_model(feats.device).flags == 3
    assert torch.equal(out["clip"][0], out["hf"][0]) and torch.equal(out["clip"][1], out["hf"][1])
    assert CH.report(name + ", hf", "features", out["hf"][0], truth["features"], rel=False)


def test_hf_gelu_variant_and_shorter_rows():
    """``hidden_act: gelu`` selects the erf epilogue (flags 2); HuggingFace's rows are as long as the longest sentence"""
    case = CC.RANK_CASES[0]
    (name, tower, seed, K, base, position) = case
    inp = CH.rank_case_inputs(case)
    truth = CH.truth_rank_case(case, inp, act="gelu")
    enc = hf_on_gpu(tower, seed, "gelu")
    pl = CH.build_learner(case, inp).cuda()
    n = int(pl.pseudo_sentence_tokens.argmax(dim=-1).max()) + 4                # positions a padding tokenizer would hand over
    sent = pl()[:, :n].detach().requires_grad_(True)
    feats = enc(prompts_embedding=sent, prompts_pseudo_tokens=pl.pseudo_sentence_tokens[:, :n])
    assert enc._c_model(feats.device).flags == 2
    ok = CH.report(name + ", hf gelu", "features", feats, truth["features"], rel=False)
    (feats * torch.from_numpy(inp["fx"]["G"]).cuda()).sum().backward()
    ok &= CH.report(name + ", hf gelu", "d prompts_embedding", sent.grad, truth["sentence"].grad[:, :n], rel=True)
    rows = CC.token_rows([5, 38, 0, 30], 11, length=40)
    with torch.no_grad():
        ok &= CH.report(name + ", hf gelu", "features (prompts_text, 40 positions)", enc(prompts_text=rows.cuda()),
                        text_truth(tower, seed, rows, "gelu"), rel=False)
    assert ok
    # the tower's own parameters never train in this layout: refused, not silently frozen
    enc.final_layer_norm.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="requires grad"):
        enc(prompts_embedding=sent, prompts_pseudo_tokens=pl.pseudo_sentence_tokens[:, :n])
    with torch.no_grad():
        enc(prompts_embedding=sent, prompts_pseudo_tokens=pl.pseudo_sentence_tokens[:, :n])


# ---- 6. the backward pass's 64-row limit ------------------------------------------------------------------------------------------------
def test_a_65_row_prompt_runs_forward_and_its_backward_is_refused():
    from vlsa_amd._native import VlsaNativeError
    tower, seed = "small", 9111
    c = CC.TOWERS[tower]
    enc = clip_on_gpu(tower, seed)
    W = CH.f64(CC.make_clip_weights(tower, seed))
    g = torch.Generator().manual_seed(65)
    for rows_of_prompt, refused in ((65, True), (62, False)):
        ms = [rows_of_prompt - 1, 9]
        pseudo = torch.zeros(2, 77, dtype=torch.long)
        for i, m in enumerate(ms):
            pseudo[i, :m + 1] = torch.arange(1, m + 2)
        emb = 0.02 * torch.randn(2, 77, c["width"], generator=g)
        G = torch.randn(2, c["out_dim"], generator=g)
        x64 = emb.double().requires_grad_(True)
        want = CH.clip_text_forward(W, c["heads"], x64, pseudo, c["layers"])
        x = emb.cuda().requires_grad_(True)
        feats = enc(prompts_embedding=x, prompts_pseudo_tokens=pseudo)
        assert enc._plan(pseudo, x.device).max_len == rows_of_prompt
        assert CH.report(f"{rows_of_prompt}-row prompt", "features", feats, want.detach(), rel=False)
        if refused:
            with pytest.raises(VlsaNativeError, match="vlsa_tt_backward"):
                (feats * G.cuda()).sum().backward()
        else:
            (feats * G.cuda()).sum().backward()
            (want * G.double()).sum().backward()
            assert CH.report(f"{rows_of_prompt}-row prompt", "d prompts_embedding", x.grad, x64.grad, rel=True)


# ---- 7. VLSA through the hooks with vlsa_api = "CLIP" ---------------------------------------------------------------------------------
def test_vlsa_built_through_the_hooks_with_the_clip_api(tmp_path):
    """The model factory end to end: ``load_model('VLSA', vlsa_api='CLIP', ...)`` reads an OpenAI-layout checkpoint from a LOCAL file
    (the default loader), builds the rank prompt learner and the prototype queries from ``text_config`` alone, and its logits over a
    seeded bag agree with the float64 truth's text features put through the existing oracle's aggregation."""
    import handler_cases as HC
    import handler_loop as HL
    from oracle import vlsa_oracle as O
    from vlsa_amd import hooks
    from vlsa_amd.model_utils import load_model
    from vlsa_amd.prompt_encoder import CLIPPromptEncoder
    tower, seed = "w512x2", 9131
    c = CC.TOWERS[tower]
    W = CC.make_clip_weights(tower, seed)
    os.makedirs(tmp_path / "openai_clip")
    torch.save(dict({k: v.half() for k, v in W.items()}, logit_scale=torch.tensor(cases.LOGIT_SCALE)), tmp_path / "openai_clip" / "ViT-B-16.pt")
    W = {k: v.half().float() for k, v in W.items()}                   # (what the checkpoint holds: fp16 values)
    table, ctx_key, rank_keys = CC.prompt_table(seed, HC.BASE_RANKS)
    gen = torch.Generator().manual_seed(seed + 7)
    protos = [f"proto{i}" for i in range(HC.P)]
    for k, n in zip(protos, (9, 14, 3, 20, 6)):
        table[k] = torch.randint(3, CC.BOS, (n,), generator=gen).tolist()
    tok = CC.ReplayTokenizer(table, CC.BOS, CC.EOS, CC.PAD, length=CC.CTX)
    prev = hooks.set_tokenizer_factory(lambda **kw: tok)
    try:
        p_init, p_proto = HC.write_prompt_files(str(tmp_path))            # (the same keys: ctx, rank0-3, proto0-4)
        cfg = HC.make_cfg(p_init, p_proto, vlsa_api="CLIP", vlsa_txt_encoder_name="ViT-B/16", path_clip_model=str(tmp_path))
        model = HL.build_model(cfg, load_model).cuda()
    finally:
        hooks.set_tokenizer_factory(prev)
    assert type(model.prompt_encoder) is CLIPPromptEncoder and model.prompt_learner.pseudo_sentence_tokens.shape == (HC.K, 77)
    state = HC.mil_state()
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected
    # truth: the learner's sentences and the prototype texts through the float64 tower, then the oracle's VLFAN + logit pooling
    W64 = CH.f64(W)
    with torch.no_grad():
        sent = model.prompt_learner().cpu().double()
    feats = CH.clip_text_forward(W64, c["heads"], sent, model.prompt_learner.pseudo_sentence_tokens.cpu(), c["layers"])
    ids = tok(protos, return_raw_tokens=False, return_num_tokens=False)
    proto = CH.clip_text_forward(W64, c["heads"], W64["token_embedding.weight"][ids], CH.eot_pseudo_tokens(ids), c["layers"])
    model.eval()
    with torch.no_grad():
        ok = CH.report("VLSA, CLIP api", "text features", model.forward_text_only(), feats, rel=False)
        ok &= CH.report("VLSA, CLIP api", "prototype features", model.mil_encoder.Q.get_raw_prompt_features(), proto, rel=False)
        Q = 0.5 * state["mil_encoder.Q.residual_features"] + proto.float()
        bags = [cases.make_bag(n, 4260 + i) for i, n in enumerate((700, 64))]
        ref = torch.cat([O.vlsa_vlfan_forward(x, Q, feats.float(), torch.tensor(cases.LOGIT_SCALE), head_weight=state["mil_encoder.visual_adapter.weight"],
                                              head_bias=state["mil_encoder.visual_adapter.bias"])["logits"] for x in bags])
        logits, _, _ = model.forward_bags([x.cuda() for x in bags])
        ok &= CH.report("VLSA, CLIP api", "bag logits", logits, ref, rel=False)
    assert ok
