"""DeepMIL TRAINING over a batch of bags (DeepMIL.forward_bags under autograd, VF.attn_pool_bags_autograd): the batched route
against the per-bag ``forward`` with autograd -- outputs and every parameter gradient --, its dropout masks (the kernels' counter-
based generator re-stated in torch, one independent seed per bag, the per-bag path's masks for a batch of one), new masks on every
step, the attention it hands back, and a captured TrainStep whose replays equal the same steps run eagerly."""
import copy

import pytest
import torch

import cases

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _model(pooling, head="default", drop=0.25, feat_proj=False, seed=3):
    from vlsa_amd.deepmil import DeepMIL
    torch.manual_seed(seed)
    m = DeepMIL(dim_in=512, dim_hid=256, num_cls=5, use_feat_proj=feat_proj, drop_rate=drop, pooling=pooling, pred_head=head,
                dim_reduction=4, keep_ratio=0.8).to(DEV)
    with torch.no_grad():                      # biases away from zero so that their gradients are not all tiny
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.add_(0.05 * torch.randn_like(p))
    return m


def _bags(sizes, dtype, seed):
    return [cases.make_bag(n, seed + i, "clustered").to(dtype).to(DEV) for i, n in enumerate(sizes)]


def _close(got, ref, what, rel=1e-4, scale=None):
    """the project's gate: 1e-4 of the reference's largest entry.  scale: for the score layer's output bias c, whose gradient is the
    sum of dL/da over a bag -- exactly zero for a softmax pooling, so both routes return fp32 cancellation noise there --, the
    largest entry of the module's other gradients"""
    tol = rel * max(ref.abs().max().item() if scale is None else scale, 1e-2)
    err = (got.float() - ref.float()).abs().max().item()
    assert err <= tol, f"{what}: max err {err:.3e} > {tol:.3e}"


def _per_bag_vs_batched(m, bags, use_bagset=True):
    from vlsa_amd import functional as VF
    ref = torch.cat([m(x[None]) for x in bags])
    G = torch.randn(ref.shape, generator=torch.Generator().manual_seed(len(bags))).to(DEV)
    (ref * G).sum().backward()
    gref = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    got = m.forward_bags(VF.BagSet(bags) if use_bagset else bags)
    (got * G).sum().backward()
    _close(got, ref, "logits", 2e-5)
    assert set(gref) == {n for n, p in m.named_parameters() if p.grad is not None}
    big = max(g.abs().max().item() for g in gref.values())
    for n, p in m.named_parameters():
        if n in gref:
            _close(p.grad, gref[n], n, scale=big if _is_c(n) else None)
    m.zero_grad(set_to_none=True)


def _is_c(name):
    return name.endswith("sigma.fc2.bias") or name.endswith("sigma.attention.2.bias")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("head", ["default", "Adapter"])
@pytest.mark.parametrize("pooling", ["gated_attention", "attention", "mean", "max"])
def test_forward_bags_equals_per_bag_forward_with_gradients(pooling, head, dtype):
    m = _model(pooling, head).eval()            # (eval: no dropout -- the two routes draw different masks)
    _per_bag_vs_batched(m, _bags([1, 37, 2798, 640, 5000, 129], dtype, 100))


@pytest.mark.parametrize("B", [1, 3, 32, 64, 65])
def test_batch_sizes_and_chunks(B):
    m = _model("gated_attention").eval()
    sizes = [1 + (173 * i) % 3000 for i in range(B)]
    _per_bag_vs_batched(m, _bags(sizes, torch.bfloat16, 200), use_bagset=(B % 2 == 1))


@pytest.mark.parametrize("pooling", ["gated_attention", "attention"])
def test_large_bags_take_the_lds_dma_score_kernel(pooling):
    from vlsa_amd import functional as VF
    bags = _bags([50000, 1, 24000, 12000], torch.bfloat16, 300)
    plan = VF.AttnBagsPlan.of(VF.BagSet(bags), pooling == "gated_attention")
    rows, _ = VF._score_big_tile(False, pooling == "gated_attention")
    assert rows and plan.rpt > VF._score_tiling(False, pooling == "gated_attention")[0]     # the LDS-DMA kernel's tile heights
    _per_bag_vs_batched(_model(pooling).eval(), bags)


def test_fp32_50k_bag_with_small_ones():
    _per_bag_vs_batched(_model("gated_attention").eval(), _bags([50000, 3, 700], torch.float32, 350))


@pytest.mark.parametrize("pooling", ["gated_attention", "attention"])
def test_trainable_feat_projecter_gets_its_gradient_through_the_batch(pooling):
    m = _model(pooling, feat_proj=True).eval()
    _per_bag_vs_batched(m, _bags([300, 2798, 1, 900], torch.bfloat16, 400), use_bagset=False)


def test_ret_with_attn_matches_per_bag():
    from vlsa_amd import functional as VF
    for pooling in ("attention", "gated_attention"):
        m = _model(pooling).eval()
        bags = _bags([10, 2798, 400], torch.bfloat16, 500)
        logits, attn = m.forward_bags(VF.BagSet(bags), ret_with_attn=True)
        for i, x in enumerate(bags):
            lg, a = m(x[None], ret_with_attn=True)
            _close(logits[i], lg[0], "logit", 2e-5)
            assert attn[i].shape == a.shape
            _close(attn[i], a, "attention", 2e-5)


def test_vlsa_forward_bags_routes_deepmil_and_returns_attention():
    from vlsa_amd.vlsa import VLSA
    cfg = dict(name="DeepMIL", dim_in=512, dim_hid=256, num_cls=512, use_feat_proj=False, drop_rate=0.25, pooling="gated_attention",
               pred_head="default")
    torch.manual_seed(4)
    net = VLSA.from_modules(cfg, pretrained_text_features=torch.randn(4, 512), logit_scale_init=cases.LOGIT_SCALE).to(DEV).eval()
    bags = _bags([120, 2798, 33], torch.bfloat16, 600)
    out = net.forward_bags(bags)
    (out[0].square().sum()).backward()
    g = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    net.zero_grad(set_to_none=True)
    ref = [net(x[None]) for x in bags]
    torch.cat([r[0] for r in ref]).square().sum().backward()
    _close(out[0], torch.cat([r[0] for r in ref]), "logits", 2e-5)
    big = max(x.abs().max().item() for x in g.values())
    for n, p in net.named_parameters():
        if n in g:
            _close(g[n], p.grad, n, scale=big if _is_c(n) else None)
    res = net.forward_bags(bags, ret_with_attn=True)
    assert len(res) == 4 and len(res[3]) == 3 and res[3][1].shape == (1, 2798)


# ---- dropout ------------------------------------------------------------------------------------------------------------------
M32 = 0xFFFFFFFF


def _mix(h):
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def _bits(seed, rows, units):
    r = torch.as_tensor(rows, dtype=torch.int64)[:, None]
    u = torch.as_tensor(units, dtype=torch.int64)[None, :]
    return _mix((seed ^ ((r * 0x9E3779B1) & M32) ^ ((u * 0x85EBCA6B) & M32)) & M32)


def _bag_seed(s, b):
    """vlsa_common.h: bag_drop_seed"""
    if b == 0:
        return s
    return int(_bits((s ^ 0x5BD1E995) & M32, [b], [M32])[0, 0])


def _weights(m):
    sg = m.sigma
    return (sg.fc1[0].weight, sg.fc1[0].bias, sg.score[0].weight, sg.score[0].bias, sg.fc2.weight, sg.fc2.bias)


def test_batched_masks_equal_the_restated_generator_for_every_bag():
    from vlsa_amd import functional as VF
    p, s = 0.25, 987654
    m = _model("gated_attention").train()
    Wa, ba, Wg, bg, w2, c = [t.detach().float().cpu() for t in _weights(m)]
    bags = _bags([700, 2798, 1, 3000, 64], torch.bfloat16, 700)
    with torch.no_grad():
        _, a = VF.attn_pool_bags_autograd(VF.BagSet(bags), VF.FusedAttnScores(), *_weights(m), drop_p=p,
                                          seed_word=torch.tensor([s], dtype=torch.int64, device=DEV))
    a, o = a.cpu(), 0
    thr = int(p * 4294967296.0)
    for b, x in enumerate(bags):
        n = x.shape[0]
        sb = _bag_seed(s, b)
        keep = (_bits(sb, range(n), range(256)) >= thr) & (_bits(sb, range(n), range(256, 512)) >= thr)
        X = x.float().cpu()
        e = torch.tanh(X @ Wa.t() + ba) * torch.sigmoid(X @ Wg.t() + bg) * keep / (1 - p) ** 2
        ref = (e @ w2.t()).squeeze(-1) + c
        _close(a[o:o + n], ref, f"scores of bag {b}", 2e-4)
        o += n


def test_batch_of_one_reproduces_the_per_bag_masks():
    from vlsa_amd import functional as VF
    p, s = 0.25, 4242
    m = _model("gated_attention").train()
    for dtype, n in ((torch.bfloat16, 2798), (torch.float32, 5000), (torch.bfloat16, 30000)):
        x = _bags([n], dtype, 800)[0]
        with torch.no_grad():
            ref = VF.attn_scores_autograd(x, VF.FusedAttnScores(), *_weights(m), drop_p=p, seed=s)
            _, a = VF.attn_pool_bags_autograd(VF.BagSet([x]), VF.FusedAttnScores(), *_weights(m), drop_p=p,
                                              seed_word=torch.tensor([s], dtype=torch.int64, device=DEV))
        _close(a, ref, f"scores {dtype} {n}", 2e-5)


def test_dropout_gradients_match_torch_with_the_same_masks():
    """train-mode batched route: every parameter gradient against torch autograd through the restated masks"""
    from vlsa_amd import functional as VF
    p, s = 0.25, 31337
    m = _model("gated_attention").train()
    bags = _bags([900, 2798, 17], torch.float32, 900)
    ws = [t.detach().clone().requires_grad_(True) for t in _weights(m)]
    dp = torch.randn(len(bags), 512, generator=torch.Generator().manual_seed(9)).to(DEV)
    pooled, _ = VF.attn_pool_bags_autograd(VF.BagSet(bags), VF.FusedAttnScores(), *ws, drop_p=p,
                                           seed_word=torch.tensor([s], dtype=torch.int64, device=DEV))
    (pooled * dp).sum().backward()
    wr = [t.detach().clone().requires_grad_(True) for t in _weights(m)]
    thr = int(p * 4294967296.0)
    outs = []
    for b, x in enumerate(bags):
        n = x.shape[0]
        sb = _bag_seed(s, b)
        keep = ((_bits(sb, range(n), range(256)) >= thr) & (_bits(sb, range(n), range(256, 512)) >= thr)).to(DEV)
        e = torch.tanh(x @ wr[0].t() + wr[1]) * torch.sigmoid(x @ wr[2].t() + wr[3]) * keep / (1 - p) ** 2
        a = (e @ wr[4].t()).squeeze(-1) + wr[5]
        outs.append(torch.softmax(a, 0) @ x)
    ref = torch.stack(outs)
    (ref * dp).sum().backward()
    _close(pooled, ref, "pooled", 2e-5)
    big = max(r.grad.abs().max().item() for r in wr)
    for i, (g, r) in enumerate(zip(ws, wr)):
        _close(g.grad, r.grad, f"param {i}", scale=big if i == 5 else None)


def test_two_consecutive_steps_draw_different_masks():
    from vlsa_amd import functional as VF
    m = _model("gated_attention").train()
    bags = VF.BagSet(_bags([2798, 500], torch.bfloat16, 1000))
    _, a1 = m.forward_bags(bags, ret_with_attn=True)
    _, a2 = m.forward_bags(bags, ret_with_attn=True)
    for x, y in zip(a1, a2):
        assert (x - y).abs().max().item() > 1e-4
    torch.manual_seed(123)                       # the counter's base comes from torch's CPU generator
    m1 = _model("gated_attention").train()
    torch.manual_seed(5)
    m1._drop_counter = None
    _, b1 = m1.forward_bags(bags, ret_with_attn=True)
    m2 = _model("gated_attention").train()
    torch.manual_seed(5)
    m2._drop_counter = None
    _, b2 = m2.forward_bags(bags, ret_with_attn=True)
    assert all(torch.equal(x, y) for x, y in zip(b1, b2))


# ---- capture ------------------------------------------------------------------------------------------------------------------
def _vlsa_deepmil():
    from vlsa_amd.vlsa import VLSA
    cfg = dict(name="DeepMIL", dim_in=512, dim_hid=256, num_cls=512, use_feat_proj=False, drop_rate=0.25, pooling="gated_attention",
               pred_head="default")
    torch.manual_seed(11)
    return VLSA.from_modules(cfg, pretrained_text_features=torch.randn(4, 512), logit_scale_init=cases.LOGIT_SCALE).to(DEV).train()


def _steps(net, graph, n, bags, t, e, frozen_pool=False, toggle=False):
    from vlsa_amd.losses import SurvObjective
    from vlsa_amd.optim import FusedAdam
    from vlsa_amd.train_step import TrainStep
    if frozen_pool:
        for p in net.mil_encoder.sigma.parameters():
            p.requires_grad_(False)
    ps = [p for p in net.parameters() if p.requires_grad]
    opt = FusedAdam([{"params": ps, "weight_decay": 0.0}], lr=1e-3)
    ts = TrainStep(net, SurvObjective(), opt, graph=graph)
    losses = []
    for i in range(n):
        losses.append(float(ts.step(bags, t, e)))
        if toggle and i % 2 == 1:
            net.eval()
            with torch.no_grad():
                net.forward_bags(bags)
            net.train()
    return losses, [p.detach().clone() for p in net.parameters()], ts


@pytest.mark.parametrize("frozen_pool", [False, True])
def test_captured_deepmil_step_replays_the_eager_steps(frozen_pool):
    from vlsa_amd import functional as VF
    bags = VF.BagSet(_bags([300 + 211 * i for i in range(8)], torch.bfloat16, 1100))
    t = torch.tensor([0, 1, 2, 3, 0, 1, 2, 0], device=DEV)
    e = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0], device=DEV)
    net_e, net_g = _vlsa_deepmil(), _vlsa_deepmil()
    ctr = torch.tensor([777], dtype=torch.int64, device=DEV)
    net_e.mil_encoder._drop_counter = ctr.clone()
    net_g.mil_encoder._drop_counter = ctr.clone()
    le, pe, _ = _steps(net_e, False, 8, bags, t, e, frozen_pool, toggle=frozen_pool)
    lg, pg, ts = _steps(net_g, True, 8, bags, t, e, frozen_pool, toggle=frozen_pool)
    d = ts.describe()
    assert d["captures"] == 1 and d["replays"] >= 5 and d["why_eager"] is None, d
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (le, lg)
    for a, b in zip(pe, pg):
        assert (a - b).abs().max().item() <= 1e-6 * max(1.0, a.abs().max().item())
    assert int(net_e.mil_encoder._drop_counter.item()) == int(net_g.mil_encoder._drop_counter.item()) == 777 + 8
    assert len(set(round(x, 9) for x in lg)) == len(lg)          # new masks (and parameters) on every replay
