"""The text tower at every sentence shape its kernels branch on (tests/text_shape_cases.py) against the float64 CPU oracle over the
full 128 positions: ragged prompts, one prompt, the attention loops at 64 / 65 / 128 rows, both sides of every row threshold of the
products and of the frozen backward's two routes, 1 .. 4 prefix keys per key workgroup and the ticketed fold, the widths 384 / 512 / 640,
a tower of three blocks, the trainable tower up to its 1024-row limit, the refusals next to the shapes that still run, and the
persistent forward at the limit of its conditions and just past each of them.

Gates (the project's): 1e-4 absolute on text features; 1e-4 of the largest entry on gradients -- per PROMPT for d embedding (a one-token
prompt's gradient is ~10x a 62-token prompt's and would hide its error), per tensor for the prefix leaf and the tower's parameters
(``1e-4 * max + 1e-7`` there, the rule of test_gpu_text_tower.py).  Yardstick: the fp32 CPU oracle's own distance from the float64 one on
these inputs, which sets each case's seed without looking at the GPU (tests/text_shape_cases.py ``SEED_STEP``) and which
tests/test_text_shape_cases_cpu.py holds to <= 2.5e-5, a quarter of the gate, for three of the cases.  Every figure is printed before it is asserted (pytest -s; profiles/r10_pytest_gpu_text_shapes.txt)."""
import pytest
import torch

import cases
import text_cases as TC
import text_shape_cases as SC
from text_helpers import count, expected_gemms_768, gemm_names, tower_kernels

pytestmark = pytest.mark.gpu
GATE = SC.GATE
# a figure that passes the gate but is more than three times the yardstick is marked "(!)" in the output: the fp32 oracle on ragged100
# is 1.2e-5 from the float64 one on features and 2.0e-5 of the prompt's largest entry on d embedding
FLAG_FEAT, FLAG_GRAD = 3 * 1.2e-5, 3 * 2.0e-5


@pytest.fixture(scope="module")
def encoders():
    """tower name (, trainable) -> encoder on the GPU; one per tower for the whole module"""
    from vlsa_amd.prompt_encoder import CONCHPromptEncoder
    cache = {}

    def get(tower, trainable=False):
        if (tower, trainable) not in cache:
            c = TC.TOWERS[tower]
            enc = CONCHPromptEncoder(width=c["width"], heads=c["heads"], layers=c["layers"], vocab_size=c["vocab"], output_dim=c["out_dim"])
            enc.load_state_dict(SC.make_weights(tower))
            for k, p in enc.named_parameters():
                p.requires_grad_(trainable and k != "token_embedding.weight")
            cache[(tower, trainable)] = enc.cuda().eval()
        return cache[(tower, trainable)]
    yield get
    cache.clear()


_REF = {}


def reference(name):
    """(inputs, float64 oracle result) of a case: computed once, shared by every test that needs it, never modified"""
    if name not in _REF:
        case = SC.get(name)
        inp = SC.make_inputs(case)
        inp["pseudo_dev"], inp["G_dev"] = inp["pseudo"].cuda(), inp["G"].cuda()
        _REF[name] = (inp, SC.oracle(case, inp, torch.float64, weight_grads=name in SC.TRAIN_CASES or name == "small_M1024",
                                     backward=case.route is not None))
    return _REF[name]


def run_hip(enc, inp, L, backward=True, grad_mode=True):
    """the encoder on the case's leaves: -> dict(feats, d_prefix, d_own, d_emb) like SC.oracle"""
    # (grad_mode False: leaves that ask for no gradient either -- the autograd function saves activations whenever its INPUT requires
    #  grad, also under no_grad -- so that this is the inference route: nothing saved, the plan's own workspace)
    prefix = inp["prefix"].cuda().requires_grad_(grad_mode) if inp["prefix"] is not None else None
    own = inp["own"].cuda().requires_grad_(grad_mode)
    emb = SC.assemble(prefix, own)
    if prefix is not None and grad_mode:
        emb.retain_grad()
    with torch.set_grad_enabled(grad_mode):
        feats = enc(prompts_embedding=emb, prompts_pseudo_tokens=inp["pseudo_dev"], shared_prefix_len=L)
    out = dict(feats=feats.detach(), d_prefix=None, d_own=None, d_emb=None, graph=feats, grad_fn=type(feats.grad_fn).__name__)
    if backward and grad_mode:
        (feats * inp["G_dev"]).sum().backward()
        out.update(d_prefix=None if prefix is None else prefix.grad, d_own=own.grad, d_emb=emb.grad, graph=None)
    return out


def feat_err(got, ref):
    return float((got["feats"].cpu().double() - ref["feats"]).abs().max())


def mark(v, flag=FLAG_GRAD):
    return f"{v:.2e}" + ("(!)" if v > flag else "")


def fmark(v):
    return mark(v, FLAG_FEAT)


def grad_checks(tag, case, got, ref, checks, plus=0.0):
    """d embedding of one backward pass against the reference: per prompt on the own rows, per tensor on the prefix leaf, exact zeros
    behind every prompt's first pad.  Appends (label, ok) to `checks`, returns the text for the case's line."""
    rel, err, scale, s = SC.per_prompt_rel(got["d_own"], ref["d_own"])
    cases.record_grad_error(f"text shapes {case.name} {tag}: d own rows, worst prompt", err, scale, GATE * scale + plus)
    checks.append((f"{tag} d own rows (prompt {s}): {err:.2e} of {scale:.2e}", err <= GATE * scale + plus))
    text = f"d own/prompt {mark(rel)} (prompt {s})"
    if ref["d_prefix"] is not None:
        rel, err, scale = SC.tensor_rel(got["d_prefix"], ref["d_prefix"])
        cases.record_grad_error(f"text shapes {case.name} {tag}: d prefix", err, scale, GATE * scale + plus)
        checks.append((f"{tag} d prefix: {err:.2e} of {scale:.2e}", err <= GATE * scale + plus))
        text += f" d prefix {mark(rel)}"
    behind = torch.arange(SC.CTX - 1)[None, :] > torch.tensor(case.lens)[:, None]        # [K, 127]: slots behind the first pad
    z = got["d_emb"][behind.cuda()]
    checks.append((f"{tag} exact zeros behind the first pad", torch.equal(z, torch.zeros_like(z))))
    return text


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_frozen_tower_at_every_shape(name, encoders):
    case = SC.get(name)
    cfg = TC.TOWERS[case.tower]
    enc = encoders(case.tower)
    inp, ref = reference(name)
    plan = enc._plan(inp["pseudo_dev"], torch.device("cuda", 0), case.L)
    checks = [("plan", (plan.M, plan.M_pad, plan.max_len, plan.prefix_len) == (case.M, case.M_pad, case.max_len, case.prefix_len))]
    bw = case.route is not None
    plan.ws = None
    f0 = run_hip(enc, inp, case.L, grad_mode=False)                                 # inference route: nothing saved
    checks.append(("inference route used the plan's workspace", plan.ws is not None))
    got = {}
    names = tower_kernels(lambda: got.update(run_hip(enc, inp, case.L, backward=bw)))     # training route
    e0, e1 = feat_err(f0, ref), feat_err(got, ref)
    checks += [(f"features, inference route: {e0:.2e}", e0 <= GATE), (f"features, training route: {e1:.2e}", e1 <= GATE)]
    line = f"features {fmark(e0)} / {fmark(e1)}"
    if bw:
        line += " " + grad_checks("", case, got, ref, checks)
        again = run_hip(enc, inp, case.L)                                           # the same plan once more: the same bits
        checks.append(("second pass bit-identical", torch.equal(again["feats"], got["feats"]) and torch.equal(again["d_emb"], got["d_emb"])))
    if case.L > 0:                                                                  # the same leaves, a row per position: same reference
        r0 = run_hip(enc, inp, 0, grad_mode=False)
        r1 = run_hip(enc, inp, 0)
        e0, e1 = feat_err(r0, ref), feat_err(r1, ref)
        checks += [(f"L=0 features, inference route: {e0:.2e}", e0 <= GATE), (f"L=0 features, training route: {e1:.2e}", e1 <= GATE)]
        line += f" | planned with L=0: features {fmark(e0)} / {fmark(e1)} " + grad_checks("L=0", case, r1, ref, checks)
    # the branch the case is there for
    gemms = gemm_names(names)
    n_attn = (count(names, r"k_tt_attn_fwd"), count(names, r"k_tt_attn_bwd"))
    checks.append((f"attention launches {n_attn}", n_attn == (cfg["layers"], cfg["layers"] if bw else 0)))
    if cfg["width"] == 768:
        want = expected_gemms_768(case.M, cfg["layers"], case.route)
        checks.append((f"products: launched {dict(gemms)}, expected {dict(want)}", gemms == want))
        has_pro = any(k.split(", ")[2] == "2" for k in gemms)
        checks.append(("LayerNorm-backward prologue present iff M <= 128", has_pro == (bw and case.M <= 128)))
        took = "forward products " + " ".join(f"<{k}>" for k in sorted(gemms) if k.split(", ")[2] == "1")
    else:
        # runtime-G products (K groups not the CONCH tower's: template argument 0), LayerNorm backward by k_tt_ln_bwd (384, 640: not a
        # multiple of 256) or k_tt_ln_bwd4 (512: two float4 slots per lane)
        checks.append((f"runtime-G products {dict(gemms)}", gemms["2, 4, 1, 0, 3"] == cfg["layers"] and all(k.split(", ")[3] == "0" for k in gemms)))
        n_ln = (count(names, r"k_tt_ln_bwd\b"), count(names, r"k_tt_ln_bwd4\b"))
        checks.append((f"LayerNorm backward launches (k_tt_ln_bwd, k_tt_ln_bwd4) {n_ln}",
                       n_ln == ((0, 2 * cfg["layers"]) if cfg["width"] == 512 else (2 * cfg["layers"], 0))))
        took = f"products {sorted(gemms)} ln_bwd {n_ln}"
    print(f"[text shapes {name}] {case.tower} K={len(case.lens)} M={plan.M} M_pad={plan.M_pad} max_len={plan.max_len} L={plan.prefix_len} "
          f"keys/wg={case.kpb} backward={case.route} {took}: {line}")
    failed = [label for label, ok in checks if not ok]
    assert not failed, failed


def test_backward_refuses_65_rows_and_the_encoder_goes_on(encoders):
    """max_len 65: the forward takes its second key chunk and is right; the attention backward holds 64 rows and the host refuses before
    any launch of it; the encoder then serves an ordinary case as before."""
    from vlsa_amd._native import VlsaNativeError
    case = SC.get("S65")
    enc = encoders(case.tower)
    inp, ref = reference("S65")
    f0 = run_hip(enc, inp, 0, grad_mode=False)
    f1 = run_hip(enc, inp, 0, backward=False)
    e0, e1 = feat_err(f0, ref), feat_err(f1, ref)
    print(f"[text shapes S65] M={case.M} max_len={case.max_len}: features {fmark(e0)} / {fmark(e1)}; backward refused")
    assert e0 <= GATE and e1 <= GATE
    with pytest.raises(VlsaNativeError):
        (f1["graph"] * inp["G_dev"]).sum().backward()
    torch.cuda.synchronize()
    other = SC.get("ragged100")
    inp, ref = reference("ragged100")
    checks = []
    got = run_hip(enc, inp, 0)
    e = feat_err(got, ref)
    print(f"[text shapes S65 -> ragged100] features {fmark(e)} " + grad_checks("after the refusal", other, got, ref, checks))
    assert e <= GATE and all(ok for _, ok in checks), checks


def close_all(tag, enc, got, ref, layers):
    """every parameter gradient of a trainable tower against the oracle's: the rule of test_gpu_text_tower.py, 1e-4 * max + 1e-7"""
    sd = dict(enc.named_parameters())
    rows, failed = [], []
    for k, want in ref["d_w"].items():
        g = sd[k].grad
        assert g is not None, k
        rel, err, scale = SC.tensor_rel(g, want)
        cases.record_grad_error(f"text shapes {tag}: {k}", err, scale, 1e-4 * scale + 1e-7)
        rows.append((rel, k))
        if not err <= 1e-4 * scale + 1e-7:
            failed.append((k, err, scale))
    assert len(rows) == 5 + 12 * layers
    worst = sorted(rows, reverse=True)[:3]
    return failed, ", ".join(f"{k} {mark(r)}" for r, k in worst)


@pytest.mark.parametrize("name", SC.TRAIN_CASES)
def test_trainable_tower_at_ragged_and_prefix_shapes(name, encoders):
    """Every tower parameter a leaf: d embedding and all 5 + 12 x layers parameter gradients (vlsa_tt_backward_train) on ragged prompts
    and with 2 and 4 prefix keys per key workgroup, widths 768, 384 and 640."""
    case = SC.get(name)
    cfg = TC.TOWERS[case.tower]
    enc = encoders(case.tower, trainable=True)
    inp, ref = reference(name)
    enc.zero_grad(set_to_none=True)
    got = run_hip(enc, inp, case.L)
    assert got["grad_fn"] == "_TextTowerTrainFnBackward"                            # the native route, not torch ops
    prefix_len = enc._plan(inp["pseudo_dev"], torch.device("cuda", 0), case.L).prefix_len
    e = feat_err(got, ref)
    failed, worst = close_all(name, enc, got, ref, cfg["layers"])
    checks = [(f"features {e:.2e}", e <= GATE), ("prefix in the plan", prefix_len == case.prefix_len)]
    text = grad_checks("trainable", case, got, ref, checks, plus=1e-7)
    print(f"[text shapes trainable {name}] {case.tower} M={case.M} L={prefix_len} keys/wg={case.kpb}: features {fmark(e)} {text}; "
          f"{5 + 12 * cfg['layers']} parameter gradients, worst: {worst}")
    assert not failed and all(ok for _, ok in checks), (failed, [l for l, ok in checks if not ok])


def test_trainable_tower_at_and_past_1024_rows(encoders):
    """kPosRowsMax: 64 prompts of 16 rows = 1024 compact rows give every parameter gradient, positional_embedding and cls_emb (the kernel
    whose row list holds 1024 entries) included; 80 prompts of 13 rows = 1040 are refused."""
    from vlsa_amd._native import VlsaNativeError
    case = SC.get("small_M1024")
    cfg = TC.TOWERS[case.tower]
    enc = encoders(case.tower, trainable=True)
    inp, ref = reference("small_M1024")
    enc.zero_grad(set_to_none=True)
    got = run_hip(enc, inp, 0)
    plan = enc._plan(inp["pseudo_dev"], torch.device("cuda", 0), 0)
    e = feat_err(got, ref)
    failed, worst = close_all("small_M1024", enc, got, ref, cfg["layers"])
    checks = [(f"features {e:.2e}", e <= GATE), ("plan", (plan.M, plan.M_pad) == (1024, 1056))]
    text = grad_checks("trainable", case, got, ref, checks, plus=1e-7)
    print(f"[text shapes trainable small_M1024] M={plan.M} M_pad={plan.M_pad}: features {fmark(e)} {text}; parameter gradients, worst: {worst}")
    assert not failed and all(ok for _, ok in checks), (failed, [l for l, ok in checks if not ok])
    past = SC.get("small_M1040")
    pin = SC.make_inputs(past)
    pin["pseudo_dev"], pin["G_dev"] = pin["pseudo"].cuda(), pin["G"].cuda()
    assert enc._plan(pin["pseudo_dev"], torch.device("cuda", 0), 0).M == 1040
    enc.zero_grad(set_to_none=True)
    f = run_hip(enc, pin, 0, backward=False)
    with pytest.raises(VlsaNativeError):
        (f["graph"] * pin["G_dev"]).sum().backward()
    torch.cuda.synchronize()
    print("[text shapes trainable small_M1040] M=1040: backward refused")


# ---- the persistent forward (VLSA_TT_PERSIST=1) ---------------------------------------------------------------------------------
def test_persistent_forward_at_the_limit_of_both_conditions(encoders, monkeypatch):
    """ragged100: 7 row tiles and max_len 64 -- the most the persistent launch takes of either.  Features with and without saved
    activations, the backward behind it, the same bits twice, and no in-kernel wait timed out."""
    case = SC.get("ragged100")
    enc = encoders(case.tower)
    inp, ref = reference("ragged100")
    monkeypatch.setenv("VLSA_TT_PERSIST", "1")
    f0 = {}
    names0 = tower_kernels(lambda: f0.update(run_hip(enc, inp, 0, grad_mode=False)))
    got = {}
    names1 = tower_kernels(lambda: got.update(run_hip(enc, inp, 0)))
    layers = TC.TOWERS[case.tower]["layers"]
    for names in (names0, names1):      # the blocks' own products (LayerNorm prologue) are gone; the text projection behind them stays
        assert count(names, "k_tt_forward_persistent") == 1 and count(names, r"k_tt_gemm<\d, \d, 1, ") == 0, names
    # without saved activations no attention launch; with them one per block behind the persistent launch (it rebuilds the row
    # statistics and the kept output the backward's key workgroups read)
    assert count(names0, "k_tt_attn_fwd") == 0 and count(names1, "k_tt_attn_fwd") == layers
    assert count(names1, "k_tt_attn_bwd") == layers
    checks = []
    e0, e1 = feat_err(f0, ref), feat_err(got, ref)
    text = grad_checks("persistent", case, got, ref, checks)
    again = run_hip(enc, inp, 0)
    print(f"[text shapes persistent ragged100] M={case.M} max_len={case.max_len}: features {fmark(e0)} / {fmark(e1)} {text}")
    assert e0 <= GATE and e1 <= GATE and all(ok for _, ok in checks), (e0, e1, checks)
    assert torch.equal(again["feats"], got["feats"]) and torch.equal(again["d_emb"], got["d_emb"])
    for pln in enc._plans.values():
        pln.check_status(wait=True)


@pytest.mark.parametrize("name", ["S65", "M113", "ones22"])
def test_persistent_forward_falls_back_past_each_condition(name, encoders, monkeypatch):
    """max_len 65 (its attention stage holds 64 rows), 113 rows (8 row tiles), 22 prompts (264 attention workgroups): asked for, the
    persistent launch must not run, and the launch-per-stage path's results are right."""
    case = SC.get(name)
    enc = encoders(case.tower)
    inp, ref = reference(name)
    bw = case.route is not None
    monkeypatch.setenv("VLSA_TT_PERSIST", "1")
    f0, got = {}, {}
    names = tower_kernels(lambda: f0.update(run_hip(enc, inp, 0, grad_mode=False)))
    names += tower_kernels(lambda: got.update(run_hip(enc, inp, 0, backward=bw)))
    assert count(names, "k_tt_forward_persistent") == 0 and count(names, "k_tt_attn_fwd") == 2 * TC.TOWERS[case.tower]["layers"], names
    checks = []
    e0, e1 = feat_err(f0, ref), feat_err(got, ref)
    text = grad_checks("fall-back", case, got, ref, checks) if bw else "(forward only)"
    print(f"[text shapes persistent asked for, {name}] M={case.M} max_len={case.max_len} K={len(case.lens)}: fell back; features {fmark(e0)} / {fmark(e1)} {text}")
    assert e0 <= GATE and e1 <= GATE and all(ok for _, ok in checks), (e0, e1, checks)
    for pln in enc._plans.values():
        pln.check_status(wait=True)
