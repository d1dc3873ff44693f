"""MaxMIL / MeanMIL TRAINING over a batch of bags: ``DeepMIL.forward_bags`` with max / mean pooling -- behind a trainable
Feat_Projecter (VF.project_max_pool_bags: the selected-row route; VF.mean_pool_bags under a row gradient) and without one -- against
the per-bag ``forward`` in logits and every parameter gradient, against the reference's own numbers (the featproj_fp_deepmil_mean /
_max fixtures, alone and inside a batch), the selected-row route against the dense one (projecter node, then VF.max_pool_bags), what
the selected-row forward keeps allocated, a captured TrainStep against the same steps run eagerly, and the FeatMIL 'max' baseline
through ``VLSA.forward_bags``."""
import gc

import numpy as np
import pytest
import torch
import torch.nn as nn

import cases
import helpers as H

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GATE = 1e-4                  # the project's gate on a gradient: this fraction of the reference tensor's largest entry
MAXMIL_CASE = ("fp_deepmil_max", "DeepMIL", 64, 0, 4, "max", 704)        # tests/golden/make_golden_maxmil.py
MEANMIL_CASE = next(c for c in cases.FEATPROJ_CASES if c[0] == "fp_deepmil_mean")


def _model(pooling, head="default", feat_proj=True, seed=3):
    from vlsa_amd.deepmil import DeepMIL
    torch.manual_seed(seed)
    m = DeepMIL(512, 256, 4, pooling=pooling, use_feat_proj=feat_proj, pred_head=head).to(DEV).eval()
    with torch.no_grad():                      # biases away from zero so that their gradients are not all tiny
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.add_(0.05 * torch.randn_like(p))
    return m


def _bags(sizes, seed, dtype=torch.float32):
    return [cases.make_bag(n, seed + i, "clustered").to(dtype).to(DEV) for i, n in enumerate(sizes)]


def _close(got, ref, what, rel=GATE):
    tol = rel * ref.abs().max().item()
    err = (got.float() - ref.float()).abs().max().item()
    print(f"{what}: max err {err:.3e}, gate {tol:.3e}")
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"


def _grads(m):
    return {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("head", ["default", "Adapter"])
@pytest.mark.parametrize("feat_proj", [True, False])
@pytest.mark.parametrize("pooling", ["max", "mean"])
def test_forward_bags_equals_per_bag_forward_with_gradients(pooling, feat_proj, head, B):
    from vlsa_amd import functional as VF
    m = _model(pooling, head, feat_proj)
    bags = _bags([1 + (173 * i) % 900 for i in range(B)], 100)
    ref = torch.cat([m(x[None]) for x in bags])
    G = torch.randn(ref.shape, generator=torch.Generator().manual_seed(B)).to(DEV)
    (ref * G).sum().backward()
    gref = _grads(m)
    m.zero_grad(set_to_none=True)
    got = m.forward_bags(VF.BagSet(bags) if B == 3 else bags)
    (got * G).sum().backward()
    _close(got, ref, "logits", 2e-5)
    assert set(gref) == set(_grads(m)) and (not feat_proj or "feat_proj.projecter.0.weight" in gref)
    for n, g in _grads(m).items():
        _close(g, gref[n], n)


class _TextParam(nn.Module):
    def __init__(self, T):
        super().__init__()
        self.T = nn.Parameter(T.clone())


def _golden_model(case):
    from vlsa_amd.vlsa import VLSA
    (name, _enc, N, P, K, pooling, seed) = case
    params = cases.make_params(max(P, 1), K, seed + 1000)
    tp = _TextParam(params["T"])
    cfg = dict(name="DeepMIL", dim_in=512, dim_hid=256, num_cls=512, use_feat_proj=True, drop_rate=0.25, pooling=pooling,
               pred_head="Adapter", dim_reduction=4, keep_ratio=0.8)
    model = VLSA.from_modules(cfg, text_provider=lambda: tp.T, prompt_learner=tp, logit_scale_init=cases.LOGIT_SCALE)
    enc = model.mil_encoder
    fpp, ad = cases.make_featproj_params(seed + 5000), cases.make_adapter_params(seed + 4000)
    with torch.no_grad():
        enc.feat_proj.projecter[0].weight.copy_(fpp["w"]); enc.feat_proj.projecter[0].bias.copy_(fpp["b"])
        enc.feat_proj.projecter[1].weight.copy_(fpp["gamma"]); enc.feat_proj.projecter[1].bias.copy_(fpp["beta"])
        enc.visual_adapter.fc[0].weight.copy_(ad["down"]); enc.visual_adapter.fc[2].weight.copy_(ad["up"])
    return model.cuda().eval(), tp


@pytest.mark.parametrize("in_batch", [False, True], ids=["alone", "in_a_batch"])
@pytest.mark.parametrize("case", [MEANMIL_CASE, MAXMIL_CASE], ids=["mean", "max"])
def test_the_references_own_numbers(case, in_batch):
    """logits and every gradient the reference's autograd produced for this bag (torch.max / torch.mean behind its Feat_Projecter),
    from ``forward_bags`` with the bag alone and between two ragged neighbours that receive no gradient"""
    (name, _enc, N, P, K, pooling, seed) = case
    fx = H.load_fixture("featproj_" + name)
    X = cases.make_bag(N, seed)
    assert np.allclose(np.array(cases.checksum(X)), fx["x_checksum"], rtol=1e-9, atol=1e-9)
    model, tp = _golden_model(case)
    Xd = X.to(DEV)
    bags = _bags([301], 900) + [Xd] + _bags([17], 901) if in_batch else [Xd]
    k = 1 if in_batch else 0
    logits, img, _ = model.forward_bags(bags)
    assert logits.shape == (len(bags), K)
    err = np.abs(logits[k:k + 1].detach().cpu().numpy() - fx["logits"]).max()
    print(f"logits: max err {err:.3e}")
    assert err < 1e-4
    assert np.abs(img.reshape(len(bags), -1)[k:k + 1].detach().cpu().numpy() - fx["image_features"]).max() < 1e-5
    (logits[k:k + 1] * H.t(fx["G"]).cuda()).sum().backward()
    enc = model.mil_encoder
    fp = enc.feat_proj.projecter
    for key, g in (("grad.fp.w", fp[0].weight.grad), ("grad.fp.b", fp[0].bias.grad), ("grad.fp.gamma", fp[1].weight.grad),
                   ("grad.fp.beta", fp[1].bias.grad), ("grad.logit_scale", model.logit_scale.grad), ("grad.T", tp.T.grad),
                   ("grad.adapter.down", enc.visual_adapter.fc[0].weight.grad), ("grad.adapter.up", enc.visual_adapter.fc[2].weight.grad)):
        print(key, cases.check_big(fx, key, g, atol=0.0, rtol=GATE))


def _projecter_weights(m):
    lin, norm = m.feat_proj.projecter[0], m.feat_proj.projecter[1]
    return lin.weight, lin.bias, norm.weight, norm.bias, norm.eps


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_selected_row_route_agrees_with_the_dense_route(dtype):
    """Feat_Projecter + max as one node over the <= 512 selected rows of a bag against the projecter node over all rows followed by
    VF.max_pool_bags (dense dX, views of one buffer: the projecter's backward takes them as they are): the same pooled rows, bit for
    bit, and dW / db / dgamma / dbeta within the gate"""
    from vlsa_amd import functional as VF
    m = _model("max")
    bags = VF.BagSet(_bags([700, 1, 2798, 65], 300, dtype))
    G = torch.randn(len(bags), 512, generator=torch.Generator().manual_seed(1)).to(DEV)
    W = _projecter_weights(m)
    dense = VF.max_pool_bags(VF.feat_project_bags(bags, VF.FusedFeatProjecter(), *W))
    (dense * G).sum().backward()
    gref = _grads(m)
    m.zero_grad(set_to_none=True)
    sel = VF.project_max_pool_bags(bags, VF.FusedFeatProjecter(), *W)
    (sel * G).sum().backward()
    assert torch.equal(sel, dense)
    assert set(gref) == set(_grads(m)) and len(gref) == 4
    for n, g in _grads(m).items():
        _close(g, gref[n], n)


def test_selected_row_forward_keeps_no_packed_rows():
    """after the forward of VF.project_max_pool_bags the node holds the selected input rows, the selected output rows (fp32
    [B * 512, 512] each), their statistics [B * 512, 4] and the result [B, 512] -- and nothing of [sum N_i, 512]"""
    from vlsa_amd import functional as VF
    m = _model("max")
    sizes = [6000, 5000]
    bags = VF.BagSet(_bags(sizes, 400, torch.bfloat16))
    W, fused, B = _projecter_weights(m), VF.FusedFeatProjecter(), len(sizes)
    with torch.no_grad():
        VF.project_max_pool_bags(bags, fused, *W)            # the packed weights, the set's tables: allocated once, kept
    VF.project_max_pool_bags(bags, fused, *W).sum().backward()
    m.zero_grad(set_to_none=True)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    out = VF.project_max_pool_bags(bags, fused, *W)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - before
    expected = 2 * B * 512 * 512 * 4 + B * 512 * 4 * 4 + B * 512 * 4
    packed = sum(sizes) * 512 * 4                             # one [sum N_i, 512] fp32 tensor
    print(f"held {held} bytes, expected {expected}, one packed tensor {packed}")
    # the caching allocator hands out a block up to 1 MiB larger than asked for rather than split it: two tensors above 1 MiB here,
    # and 64 KiB for the 512-byte rounding of the small ones
    slack = 2 * (1 << 20) + 65536
    assert expected + slack < packed
    assert expected <= held <= expected + slack, (held, expected)
    del out


def _vlsa_maxmil():
    from vlsa_amd.vlsa import VLSA
    cfg = dict(name="DeepMIL", dim_in=512, dim_hid=256, num_cls=512, use_feat_proj=True, drop_rate=0.25, pooling="max", pred_head="default")
    torch.manual_seed(11)
    return VLSA.from_modules(cfg, pretrained_text_features=torch.randn(4, 512), logit_scale_init=cases.LOGIT_SCALE).to(DEV).train()


def _steps(net, graph, n, bags, t, e):
    from vlsa_amd.losses import SurvObjective
    from vlsa_amd.optim import FusedAdam
    from vlsa_amd.train_step import TrainStep
    ps = [p for p in net.parameters() if p.requires_grad]
    ts = TrainStep(net, SurvObjective(), FusedAdam([{"params": ps, "weight_decay": 0.0}], lr=1e-3), graph=graph)
    losses = [float(ts.step(bags, t, e)) for _ in range(n)]
    return losses, [p.detach().clone() for p in net.parameters()], ts


def test_captured_maxmil_step_replays_the_eager_steps():
    from vlsa_amd import functional as VF
    bags = VF.BagSet(_bags([300 + 211 * i for i in range(8)], 1100, torch.bfloat16))
    t = torch.tensor([0, 1, 2, 3, 0, 1, 2, 0], device=DEV)
    e = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0], device=DEV)
    net_e, net_g = _vlsa_maxmil(), _vlsa_maxmil()
    assert any(p.requires_grad for p in net_e.mil_encoder.feat_proj.parameters())
    le, pe, _ = _steps(net_e, False, 8, bags, t, e)
    lg, pg, ts = _steps(net_g, True, 8, bags, t, e)
    d = ts.describe()
    assert d["captures"] == 1 and d["replays"] >= 5 and d["why_eager"] is None, d
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (le, lg)
    for a, b in zip(pe, pg):
        assert (a - b).abs().max().item() <= 1e-6 * max(1.0, a.abs().max().item())
    assert len(set(round(x, 9) for x in lg)) == len(lg)          # the parameters moved on every replay
    w0 = _vlsa_maxmil().mil_encoder.feat_proj.projecter[0].weight
    assert (net_g.mil_encoder.feat_proj.projecter[0].weight - w0).abs().max().item() > 1e-4      # the projecter trained


@pytest.mark.parametrize("B", [1, 3, 65])
def test_vlsa_featmil_max_equals_the_per_bag_stack(B):
    from vlsa_amd.vlsa import VLSA
    torch.manual_seed(5)
    net = VLSA.from_modules(dict(name="FeatMIL", dim_in=512, pooling="max"), pretrained_text_features=torch.randn(4, 512),
                            logit_scale_init=cases.LOGIT_SCALE).to(DEV).eval()
    bags = _bags([1 + (331 * i) % 1500 for i in range(B)], 1200, torch.bfloat16)
    with torch.no_grad():
        logits, feats, _ = net.forward_bags(bags)
        ref = [net(x[None]) for x in bags]
    _close(feats, torch.cat([r[1] for r in ref]), "features", 2e-6)
    _close(logits, torch.cat([r[0] for r in ref]), "logits", 2e-5)
