"""The CLIP text towers (QuickGELU, the <eot> row pooled) at width 768 and at every sentence shape the kernels branch on
(tests/clip_shape_cases.py) against the float64 truth ``clip_text_helpers.clip_text_forward`` over the full 77 positions: ragged prompts,
one prompt, a two-row prompt, the attention loops at 64 / 65 / 66 / 77 rows, both sides of every row threshold of the products and of the
frozen backward's two routes, 1 .. 4 prefix keys per key workgroup and the ticketed fold, a tower of three blocks, the 768-wide
projection, the trainable tower, the HuggingFace layout on rows shorter than 77 positions, and the persistent forward's refusal of a
tower that is not the CoCa one.  The counterpart of tests/test_gpu_text_tower_shapes.py; every static-G QuickGELU instantiation of
k_tt_gemm (``REQUIRED``) is launched by at least one case.

Gates (the project's): 1e-4 absolute on text features; 1e-4 of the largest entry on gradients -- per PROMPT for d embedding, per tensor
(``1e-4 * max + 1e-7``) for the prefix leaf and the tower's parameters.  Yardstick: the fp32 CPU truth's own distance from the float64 one
on these inputs, which sets each case's seed without looking at the GPU (tests/clip_shape_cases.py ``SEED_STEP``) and which
tests/test_clip_shape_cases_cpu.py holds to <= 2.5e-5 for three of the cases.  Every figure is printed before it is asserted
(pytest -s; profiles/r18_pytest_gpu_clip_shapes.txt)."""
import pytest
import torch

import cases
import clip_shape_cases as SC
import clip_text_cases as CC
import clip_text_helpers as CH
from text_helpers import count, expected_gemms_768, gemm_names, tower_kernels

pytestmark = pytest.mark.gpu
GATE = SC.GATE
FLAG = 3 * SC.YARDSTICK_MAX     # a figure that passes the gate but is more than three times the yardstick is marked "(!)" in the output
# the QuickGELU products with compile-time K groups (width 768) that no narrower tower reaches: c_fc forward (PRO 5), d h_pre (PRO 4) at the
# three tile shapes, d h_pre behind a LayerNorm-backward prologue (PRO 6)
REQUIRED = ["1, 4, 5, 12, 6", "2, 4, 5, 12, 4", "3, 4, 5, 12, 3", "1, 4, 4, 12, 6", "2, 4, 4, 12, 4", "3, 4, 4, 12, 3", "1, 4, 6, 12, 6"]


@pytest.fixture(scope="module")
def encoders():
    """(tower, layout, trainable, hidden_act) -> encoder on the GPU; one each for the whole module"""
    from vlsa_amd.prompt_encoder import HFCLIPPromptEncoder
    cache = {}

    def get(tower, layout="clip", trainable=False, act="quick_gelu"):
        key = (tower, layout, trainable, act)
        if key not in cache:
            if layout == "clip":
                enc = CH.clip_encoder(tower, SC.TOWER_SEEDS[tower])
                for k, p in enc.named_parameters():
                    p.requires_grad_(trainable and k != "token_embedding.weight")
            else:
                enc = HFCLIPPromptEncoder(CH.hf_model(tower, SC.TOWER_SEEDS[tower], act))
                for p in enc.parameters():
                    p.requires_grad_(False)
            cache[key] = enc.cuda().eval()
        return cache[key]
    yield get
    cache.clear()


_REF = {}
_NAMES = {}      # case -> kernel names of its training-route pass through the frozen tower (test 1)


def reference(name, act="quick_gelu"):
    """(inputs, float64 truth) of a case: computed once, shared by every test that needs it, never modified"""
    if (name, act) not in _REF:
        case = SC.get(name)
        inp = SC.make_inputs(case)
        inp["pseudo_dev"], inp["G_dev"] = inp["pseudo"].cuda(), inp["G"].cuda()
        _REF[(name, act)] = (inp, SC.truth(case, inp, torch.float64, weight_grads=name in SC.TRAIN_CASES, backward=case.route is not None,
                                           act=act))
    return _REF[(name, act)]


def run_hip(enc, inp, L, backward=True, grad_mode=True, n=SC.CTX):
    """the encoder on the case's leaves, cut to the first ``n`` positions: -> dict(feats, d_prefix, d_own, d_emb) like SC.truth"""
    # (grad_mode False: leaves that ask for no gradient either, so that this is the inference route: nothing saved, the plan's workspace)
    prefix = inp["prefix"].cuda().requires_grad_(grad_mode) if inp["prefix"] is not None else None
    own = inp["own"][:, :n - (0 if prefix is None else prefix.shape[0])].contiguous().cuda().requires_grad_(grad_mode)
    emb = SC.assemble(prefix, own)
    if prefix is not None and grad_mode:
        emb.retain_grad()
    with torch.set_grad_enabled(grad_mode):
        feats = enc(prompts_embedding=emb, prompts_pseudo_tokens=inp["pseudo_dev"][:, :n], shared_prefix_len=L)
    out = dict(feats=feats.detach(), d_prefix=None, d_own=None, d_emb=None, grad_fn=type(feats.grad_fn).__name__, emb=emb.detach())
    if backward and grad_mode:
        (feats * inp["G_dev"]).sum().backward()
        out.update(d_prefix=None if prefix is None else prefix.grad, d_own=own.grad, d_emb=emb.grad)
    return out


def feat_err(got, ref):
    return float((got["feats"].cpu().double() - ref["feats"]).abs().max())


def mark(v):
    return f"{v:.2e}" + ("(!)" if v > FLAG else "")


def grad_checks(tag, case, got, ref, checks):
    """d embedding of one backward pass against the truth: per prompt on the own rows, per tensor on the prefix leaf, exact zeros behind
    every prompt's <eot>.  Appends (label, ok) to `checks`, returns the text for the case's line."""
    n_own = got["d_own"].shape[1]
    rel, err, scale, s = SC.per_prompt_rel(got["d_own"], ref["d_own"][:, :n_own])
    cases.record_grad_error(f"clip shapes {case.name} {tag}: d own rows, worst prompt", err, scale, GATE * scale)
    checks.append((f"{tag} d own rows (prompt {s}): {err:.2e} of {scale:.2e}", err <= GATE * scale))
    text = f"d own/prompt {mark(rel)} (prompt {s})"
    if ref["d_prefix"] is not None:
        rel, err, scale = SC.tensor_rel(got["d_prefix"], ref["d_prefix"])
        cases.record_grad_error(f"clip shapes {case.name} {tag}: d prefix", err, scale, GATE * scale + 1e-7)
        checks.append((f"{tag} d prefix: {err:.2e} of {scale:.2e}", err <= GATE * scale + 1e-7))
        text += f" d prefix {mark(rel)}"
    behind = torch.arange(got["d_emb"].shape[1])[None, :] >= torch.tensor(case.rows)[:, None]          # slots behind <eot>
    z = got["d_emb"][behind.cuda()]
    checks.append((f"{tag} exact zeros behind <eot>", torch.equal(z, torch.zeros_like(z))))
    eot = torch.stack([got["d_emb"][s, r - 1] for s, r in enumerate(case.rows)])
    checks.append((f"{tag} a gradient on every <eot> slot", bool(eot.abs().amax(dim=1).gt(0).all())))
    return text


# ---- 1. the frozen tower at every case ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_frozen_clip_tower_at_every_shape(name, encoders):
    case = SC.get(name)
    cfg = CC.TOWERS[case.tower]
    enc = encoders(case.tower)
    inp, ref = reference(name)
    plan = enc._plan(inp["pseudo_dev"], torch.device("cuda", 0), case.L)
    checks = [("plan", (plan.M, plan.M_pad, plan.max_len, plan.prefix_len) == (case.M, case.M_pad, case.max_len, case.prefix_len)),
              (f"largest activation input {ref['stats']['act_input_absmax']:.2f} > 6", ref["stats"]["act_input_absmax"] > 6.0),
              ("flags: QuickGELU, <eot> pooling", enc._c_model(torch.device("cuda", 0)).flags == 3)]
    bw = case.route is not None
    plan.ws = None
    f0 = run_hip(enc, inp, case.L, grad_mode=False)                                 # inference route: nothing saved
    checks.append(("inference route used the plan's workspace", plan.ws is not None))
    got = {}
    names = tower_kernels(lambda: got.update(run_hip(enc, inp, case.L, backward=bw)))     # training route
    _NAMES[name] = names
    e0, e1 = feat_err(f0, ref), feat_err(got, ref)
    checks += [(f"features, inference route: {e0:.2e}", e0 <= GATE), (f"features, training route: {e1:.2e}", e1 <= GATE)]
    line = f"features {mark(e0)} / {mark(e1)}"
    if bw:
        checks.append(("the native backward", got["grad_fn"] == "_TextTowerFnBackward"))
        line += " " + grad_checks("", case, got, ref, checks)
        again = run_hip(enc, inp, case.L)                                           # the same plan once more: the same bits
        checks.append(("second pass bit-identical", torch.equal(again["feats"], got["feats"]) and torch.equal(again["d_emb"], got["d_emb"])))
    if case.L > 0:                                                                  # the same leaves, a row per position: same truth
        r0 = run_hip(enc, inp, 0, grad_mode=False)
        r1 = run_hip(enc, inp, 0)
        e0, e1 = feat_err(r0, ref), feat_err(r1, ref)
        checks += [(f"L=0 features, inference route: {e0:.2e}", e0 <= GATE), (f"L=0 features, training route: {e1:.2e}", e1 <= GATE)]
        line += f" | planned with L=0: features {mark(e0)} / {mark(e1)} " + grad_checks("L=0", case, r1, ref, checks)
    # the branch the case is there for
    gemms = gemm_names(names)
    n_attn = (count(names, r"k_tt_attn_fwd"), count(names, r"k_tt_attn_bwd"))
    checks.append((f"attention launches {n_attn}", n_attn == (cfg["layers"], cfg["layers"] if bw else 0)))
    want = expected_gemms_768(case.M, cfg["layers"], case.route, "quick_gelu", cfg["out_dim"])
    checks.append((f"products: launched {dict(gemms)}, expected {dict(want)}", gemms == want))
    has_pro6 = any(k.split(", ")[2] == "6" for k in gemms)
    checks.append(("QuickGELU behind a LayerNorm-backward prologue present iff backward and M <= 128", has_pro6 == (bw and case.M <= 128)))
    if bw:      # d prompts_embedding: written by the pass's last LayerNorm backward on the fused route, else memset + scatter
        n_sc = (count(names, r"k_tt_ln_bwd4"), count(names, r"k_tt_scatter"))
        checks.append((f"(k_tt_ln_bwd4, k_tt_scatter) launches {n_sc}",
                       n_sc == ((1, 0) if case.route == "fused" else (2 * cfg["layers"], 1))))
        checks.append(("k_tt_tile_rows in front of the d pooled product iff out_dim 768", count(names, r"k_tt_tile_rows") == (cfg["out_dim"] == 768)))
    took = "QuickGELU products " + " ".join(f"<{k}>" for k in sorted(gemms) if k.split(", ")[2] in "456")
    print(f"[clip shapes {name}] {case.tower} K={len(case.rows)} M={plan.M} M_pad={plan.M_pad} max_len={plan.max_len} L={plan.prefix_len} "
          f"keys/wg={case.kpb} backward={case.route} {took}: {line}")
    print(f"[clip shapes {name}] products launched: {dict(sorted(gemms.items()))}")
    failed = [label for label, ok in checks if not ok]
    assert not failed, failed


def test_every_static_g_quickgelu_product_was_launched(encoders):
    """The union over the table's cases holds every ``REQUIRED`` instantiation.  (A case the frozen-tower test has not run in this
    process -- a selection with -k -- is launched here, unchecked, for its kernel names alone.)"""
    for case in SC.CASES:
        if case.name not in _NAMES:
            inp, _ = reference(case.name)
            _NAMES[case.name] = tower_kernels(lambda: run_hip(encoders(case.tower), inp, case.L, backward=case.route is not None))
    by = {k: sorted(n for n, names in _NAMES.items() if k in gemm_names(names)) for k in REQUIRED}
    for k in REQUIRED:
        print(f"[clip shapes] k_tt_gemm<{k}> launched by: {' '.join(by[k]) or '-'}")
    assert all(by[k] for k in REQUIRED), {k: v for k, v in by.items() if not v}


# ---- 2. the trainable tower -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.TRAIN_CASES)
def test_trainable_clip_tower_at_ragged_and_prefix_shapes(name, encoders):
    """Every tower parameter but the token embedding a leaf: d embedding and all 4 + 12 x layers parameter gradients
    (vlsa_tt_backward_train; positional_embedding among them, no cls_emb) on ragged prompts of either row count class and with 2 and 4
    prefix keys per key workgroup."""
    case = SC.get(name)
    cfg = CC.TOWERS[case.tower]
    enc = encoders(case.tower, trainable=True)
    inp, ref = reference(name)
    enc.zero_grad(set_to_none=True)
    got = {}
    names = tower_kernels(lambda: got.update(run_hip(enc, inp, case.L)))
    assert got["grad_fn"] == "_TextTowerTrainFnBackward"                            # the native route, not torch ops
    prefix_len = enc._plan(inp["pseudo_dev"], torch.device("cuda", 0), case.L).prefix_len
    e = feat_err(got, ref)
    params = dict(enc.named_parameters())
    assert "cls_emb" not in params and "positional_embedding" in ref["d_w"] and params["token_embedding.weight"].grad is None
    rows, failed = [], []
    for k, want in ref["d_w"].items():
        assert params[k].grad is not None, k
        rel, err, scale = SC.tensor_rel(params[k].grad, want)
        cases.record_grad_error(f"clip shapes trainable {name}: {k}", err, scale, 1e-4 * scale + 1e-7)
        rows.append((rel, k))
        if not err <= 1e-4 * scale + 1e-7:
            failed.append((k, err, scale))
    assert len(rows) == 4 + 12 * cfg["layers"]
    worst = ", ".join(f"{k} {mark(r)}" for r, k in sorted(rows, reverse=True)[:3])
    gemms = gemm_names(names)
    dh = "1, 4, 4, 12, 6" if case.M <= 128 else "2, 4, 4, 12, 4"                    # d h_pre, a launch per stage: no prologue variant
    checks = [(f"features {e:.2e}", e <= GATE), ("prefix in the plan", prefix_len == case.prefix_len),
              (f"d h_pre products {dict(gemms)}", gemms[dh] == cfg["layers"] and not any(k.split(", ")[2] in "26" for k in gemms))]
    text = grad_checks("trainable", case, got, ref, checks)
    print(f"[clip shapes trainable {name}] {case.tower} M={case.M} L={prefix_len} keys/wg={case.kpb}: features {mark(e)} {text}; "
          f"{len(rows)} parameter gradients, worst: {worst}")
    assert not failed and all(ok for _, ok in checks), (failed, [l for l, ok in checks if not ok])


# ---- 3. the HuggingFace layout: rows as long as the longest sentence, the 768-wide projection -------------------------------------------
@pytest.mark.parametrize("name,act", SC.HF_CASES, ids=[f"{n}-{a}" for n, a in SC.HF_CASES])
def test_hf_layout_on_rows_shorter_than_77_positions(name, act, encoders):
    """``HFCLIPPromptEncoder`` frozen, its rows cut to max m + 4 positions: d prompts_embedding is then a [K, n, 768] block with n < 77
    that the pass's last LayerNorm backward writes itself (no scatter launch); the d pooled product of a 768-wide projection.  With
    QuickGELU the same bits as the OpenAI layout on the same rows; with ``hidden_act: gelu`` the erf epilogue under <eot> pooling."""
    case = SC.get(name)
    cfg = CC.TOWERS[case.tower]
    enc = encoders(case.tower, layout="hf", act=act)
    inp, ref = reference(name, act)
    n = max(case.rows) + 3                                                          # <eot> at m = r - 1: positions 0 .. m + 3
    assert n < SC.CTX and enc._c_model(torch.device("cuda", 0)).flags == (3 if act == "quick_gelu" else 2)
    f0 = run_hip(enc, inp, case.L, grad_mode=False, n=n)
    got = {}
    names = tower_kernels(lambda: got.update(run_hip(enc, inp, case.L, n=n)))
    plan = enc._plan(inp["pseudo_dev"][:, :n], torch.device("cuda", 0), case.L)
    gemms = gemm_names(names)
    e0, e1 = feat_err(f0, ref), feat_err(got, ref)
    checks = [("plan", (plan.M, plan.max_len, plan.prefix_len) == (case.M, case.max_len, case.prefix_len)),
              (f"features, inference route: {e0:.2e}", e0 <= GATE), (f"features, training route: {e1:.2e}", e1 <= GATE),
              ("d embedding written by the last LayerNorm backward", (count(names, r"k_tt_ln_bwd4"), count(names, r"k_tt_scatter")) == (1, 0)),
              (f"products {dict(gemms)}", gemms == expected_gemms_768(case.M, cfg["layers"], case.route, act, cfg["out_dim"])),
              ("k_tt_tile_rows in front of the d pooled product", count(names, r"k_tt_tile_rows") == 1)]
    text = grad_checks(f"hf {act}", case, got, ref, checks)
    if act == "quick_gelu":                                                         # the OpenAI layout takes 77 positions: zeros behind the cut
        clip = encoders(case.tower)
        x = torch.cat([got["emb"], torch.zeros(len(case.rows), SC.CTX - n, cfg["width"], device="cuda")], dim=1).requires_grad_(True)
        feats = clip(prompts_embedding=x, prompts_pseudo_tokens=inp["pseudo_dev"], shared_prefix_len=case.L)
        (feats * inp["G_dev"]).sum().backward()
        checks.append(("bit-equal to the OpenAI layout", torch.equal(feats.detach(), got["feats"]) and torch.equal(x.grad[:, :n], got["d_emb"])
                       and not x.grad[:, n:].any()))
    print(f"[clip shapes hf {name} {act}] {n} positions, M={plan.M} L={plan.prefix_len}: features {mark(e0)} / {mark(e1)} {text}")
    failed = [label for label, ok in checks if not ok]
    assert not failed, failed


# ---- 4. the persistent forward knows the CoCa tower only --------------------------------------------------------------------------------
def test_persistent_forward_is_not_taken_for_a_clip_tower(encoders, monkeypatch):
    """ragged100 meets every shape condition of the persistent launch (7 row tiles, max_len 64, 4 x 12 attention workgroups); with
    VLSA_TT_PERSIST=1 asked for, a tower with flags != 0 must still run launch per stage, and be right."""
    case = SC.get("ragged100")
    layers = CC.TOWERS[case.tower]["layers"]
    enc = encoders(case.tower)
    inp, ref = reference("ragged100")
    monkeypatch.setenv("VLSA_TT_PERSIST", "1")
    f0, got = {}, {}
    names0 = tower_kernels(lambda: f0.update(run_hip(enc, inp, 0, grad_mode=False)))
    names1 = tower_kernels(lambda: got.update(run_hip(enc, inp, 0)))
    for names in (names0, names1):
        assert count(names, "k_tt_forward_persistent") == 0 and count(names, "k_tt_attn_fwd") == layers, names
        assert gemm_names(names)["1, 4, 5, 12, 6"] == layers
    checks = []
    e0, e1 = feat_err(f0, ref), feat_err(got, ref)
    text = grad_checks("persistent asked for", case, got, ref, checks)
    print(f"[clip shapes persistent asked for, ragged100] M={case.M} max_len={case.max_len}: launch per stage; features {mark(e0)} / {mark(e1)} {text}")
    assert e0 <= GATE and e1 <= GATE and all(ok for _, ok in checks), (e0, e1, checks)
    for pln in enc._plans.values():
        pln.check_status(wait=True)
