"""The differentiable zero-shot route on the GPU (prompt pre-training: identity FeatMIL + logit pooling with trainable text features):
``VF.zeroshot_pool_bags`` under grad and ``VLSA.forward_bags`` on top of it, against ``oracle.vlsa_oracle.vlsa_zeroshot_forward`` in
float64 under autograd (on the bf16-rounded values for bf16 bags).  Logits within 1e-4, every gradient within 1e-4 of the largest entry
of its reference; the three new entry points on their own; ``TrainStep`` eager and captured over a ``BagSet``."""
import numpy as np
import pytest
import torch

import cases
import zeroshot_train_cases as Z

pytestmark = pytest.mark.gpu


def _gpu_bags(batch, dt):
    return [x.cuda() for x in Z.bags_of(batch, dt)]


def _pool(bags, T, ls, k, G):
    from vlsa_amd import functional as VF
    T = T.clone().cuda().requires_grad_(True)
    ls = ls.clone().cuda().requires_grad_(True)
    logits = torch.cat([VF.zeroshot_pool_bags(bags[i:i + 64], T, ls, k) for i in range(0, len(bags), 64)])
    (logits * G.cuda()).sum().backward()
    return logits.detach(), T.grad, ls.grad


def _check(what, got, ref):
    logits, dT, dls = (t.double().cpu() for t in got)
    rl, rT, rs = ref
    e_l, e_T, e_s = float((logits - rl).abs().max()), float((dT - rT).abs().max()), abs(float(dls) - float(rs))
    m_T, m_s = float(rT.abs().max()), abs(float(rs))
    print(f"{what}: logits {e_l:.2e}  dT {e_T:.2e} / max {m_T:.2e}  dls {e_s:.2e} / {m_s:.2e}")
    cases.record_grad_error("zeroshot dT " + what, e_T, m_T, 1e-4 * m_T)
    cases.record_grad_error("zeroshot dls " + what, e_s, m_s, 1e-4 * m_s)
    assert e_l < 1e-4
    assert e_T < 1e-4 * m_T
    assert e_s < 1e-4 * m_s


@pytest.mark.parametrize("case", Z.CASES, ids=lambda c: "-".join(map(str, c)))
def test_logits_and_gradients_equal_the_oracle(case):
    batch, K, dt, pooling = case
    k, seed = Z.topk_of(pooling), Z.SEEDS[case]
    T = Z.text_of(K, seed)
    if k is not None:          # a near-tie at the k-th place would make the selected set ill-defined: asserted, not skipped
        assert Z.min_gap(Z.bags_of(batch, dt), T, k) >= Z.GAP
    bags = _gpu_bags(batch, dt)
    got = _pool(bags, T, torch.tensor(cases.LOGIT_SCALE), k, Z.upstream_of(len(bags), K, seed))
    _check("-".join(map(str, case)), got, Z.reference(*case))


def _tied_bag(dtype):
    X = cases.make_bag(24, 8800, "iid").to(dtype)
    return torch.cat([X, X[:13]])                # rows n and n + 24 are equal for n < 13


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("pooling", ["logit_top3", "logit_top10"])
def test_exact_ties_match_the_oracle_and_the_lower_row_comes_first(dtype, pooling):
    """duplicated rows: equal cosines and equal unit rows, so whichever of a pair is pooled the gradient is the oracle's"""
    from oracle import vlsa_oracle as O
    from vlsa_amd import functional as VF
    k, K = Z.topk_of(pooling), 4
    X = _tied_bag(dtype)
    T = torch.randn(K, 512, generator=cases.gen(8801))
    G = torch.randn(1, K, generator=cases.gen(8802))
    Td = T.double().requires_grad_(True)
    ls = torch.tensor(cases.LOGIT_SCALE, dtype=torch.float64, requires_grad=True)
    # the precondition on the DISTINCT rows: an exact tie may straddle the k-th place (equal unit rows: same gradient), a near-tie not
    c = torch.sort(O.l2_normalize(T.double()) @ O.l2_normalize(X.double()).t(), dim=1, descending=True).values
    below = torch.where(c < c[:, k - 1:k] - 1e-12, c, torch.full_like(c, -2.0)).max(1).values
    assert float((c[:, k - 1] - below).min()) >= Z.GAP
    ref = O.vlsa_zeroshot_forward(X.double(), Td, ls, pooling)[0]
    (ref * G.double()).sum().backward()
    _check(f"ties-{pooling}", _pool([X.cuda()], T, torch.tensor(cases.LOGIT_SCALE), k, G), (ref.detach(), Td.grad, ls.grad))
    # the indices the backward gathered: where two pooled rows are the same row of the original bag, the lower one comes first
    table = VF._BagTable([X.cuda()])
    vals, idx, scores = _select(table, T.cuda(), k)
    idx, c = idx[0].cpu().numpy(), scores[0].cpu().numpy()
    pairs = 0
    for j in range(K):
        for a in range(k - 1):
            if c[j, idx[j, a]] == c[j, idx[j, a + 1]]:
                assert idx[j, a] < idx[j, a + 1]
                pairs += idx[j, a + 1] == idx[j, a] + 24
    assert pairs >= 1                            # the duplicated rows do score equal on the GPU: the tie rule was exercised


def _select(table, T, k, with_mean=False):
    """the streaming score launch + vlsa_topk_select_batch (and vlsa_topk_mean_batch) on a bag table: (vals, idx, score views[, mean vals])"""
    from vlsa_amd import _native as nat, functional as VF
    lib, s = nat.load(), VF._stream()
    P, B, dev = T.shape[0], table.B, table.desc.device
    qp = VF.prepare_queries(T, False, 1.0 / 1.4426950408889634)
    sc = VF.AttnBuffers(table.sizes, P, dev)
    ws = torch.empty(lib.vlsa_batch_workspace_bytes(B, P, 512), dtype=torch.uint8, device=dev)
    nat.check(lib.vlsa_vlfan_partial_batch_scores(VF._p(table.desc), B, table.dt, 512, VF._p(qp.buf), P, VF._p(ws), 0, table.groups(0),
                                                  VF._p(sc.desc), s), "scores")
    ls = torch.tensor([cases.LOGIT_SCALE], device=dev)
    vals = torch.full((B, P), float("nan"), device=dev)
    idx = torch.full((B, P, max(k or 1, 1)), -7, dtype=torch.int32, device=dev)
    nat.check(lib.vlsa_topk_select_batch(VF._p(table.desc), VF._p(sc.desc), B, P, k or 0, VF._p(ls), VF._p(vals), VF._p(idx), s), "select")
    if not with_mean:
        return vals, idx, sc.views
    mean = torch.full((B, P), float("nan"), device=dev)
    nat.check(lib.vlsa_topk_mean_batch(VF._p(table.desc), VF._p(sc.desc), B, P, k or 0, VF._p(ls), VF._p(mean), s), "mean")
    return vals, idx, sc.views, mean


@pytest.mark.parametrize("dt", Z.DTYPES)
@pytest.mark.parametrize("k", [1, 3, 10, 32, None])
def test_topk_select_batch_alone(dt, k):
    from vlsa_amd import functional as VF
    bags = _gpu_bags("ragged", dt)
    table = VF._BagTable(bags)
    vals, idx, views, mean = _select(table, Z.text_of(12, 8900).cuda(), k, with_mean=True)
    assert torch.equal(vals, mean)                                           # bit for bit the pooled values of vlsa_topk_mean_batch
    if k is None:
        assert bool((idx == -7).all())                                       # the mean over all patches writes no index
        return
    scale = float(np.exp(np.float32(cases.LOGIT_SCALE)))
    for b, n in enumerate(Z.RAGGED):
        m, c, ib = min(k, n), views[b].cpu(), idx[b].cpu().long()
        assert bool((ib[:, m:] == -1).all())                                 # slots past N_b
        win = ib[:, :m]
        assert bool(((win >= 0) & (win < n)).all())
        for j in range(win.shape[0]):
            assert len(set(win[j].tolist())) == m                            # distinct
        picked = torch.gather(c, 1, win)
        assert bool((picked[:, :-1] >= picked[:, 1:]).all())                 # descending score ...
        tie = picked[:, :-1] == picked[:, 1:]
        assert bool((win[:, :-1] < win[:, 1:])[tie].all())                   # ... ascending row among equals
        rest = c.clone().scatter_(1, win, float("-inf"))
        assert bool((rest.max(1).values <= picked[:, -1]).all())             # nothing larger was left behind
        pooled = picked.double().mean(1) * scale
        assert float((pooled - vals[b].cpu().double()).abs().max()) < 1e-5 * max(1.0, float(pooled.abs().max()))


@pytest.mark.parametrize("dt", Z.DTYPES)
def test_unit_mean_batch(dt):
    """the ragged batch (N = 1 included) plus a bag with an all-zero row (x / max(|x|, 1e-12) = 0): float64 unit-row means within 1e-6"""
    from vlsa_amd import _native as nat, functional as VF
    lib = nat.load()
    bags = list(Z.bags_of("ragged", dt))
    Xz = cases.make_bag(70, 8950, "iid").to(bags[0].dtype)
    Xz[17] = 0
    bags.append(Xz)
    dev_bags = [x.cuda() for x in bags]
    table = VF._BagTable(dev_bags)
    u = torch.full((table.B, 512), float("nan"), device="cuda")
    outs = []
    for _ in range(2):
        ws = torch.empty(lib.vlsa_unit_mean_workspace_bytes(table.B), dtype=torch.uint8, device="cuda")
        nat.check(lib.vlsa_unit_mean_batch(VF._p(table.desc), table.B, table.dt, 512, VF._p(ws), VF._p(u), VF._stream()), "unit_mean")
        outs.append(u.clone())
    assert torch.equal(outs[0], outs[1])                                     # fixed-order sums: bit-reproducible
    for b, X in enumerate(bags):
        Xd = X.double()
        ref = (Xd / Xd.norm(dim=1, keepdim=True).clamp_min(1e-12)).mean(0)
        assert float((u[b].cpu().double() - ref).abs().max()) < 1e-6, (b, X.shape[0])
    # a bag's mean does not depend on the batch it is in
    t1 = VF._BagTable(dev_bags[4:5])
    u1 = torch.empty(1, 512, device="cuda")
    ws = torch.empty(lib.vlsa_unit_mean_workspace_bytes(1), dtype=torch.uint8, device="cuda")
    nat.check(lib.vlsa_unit_mean_batch(VF._p(t1.desc), 1, t1.dt, 512, VF._p(ws), VF._p(u1), VF._stream()), "unit_mean")
    assert torch.equal(u1[0], u[4])


@pytest.mark.parametrize("pooling", ["logit_top10", "logit_mean"])
def test_grad_route_is_bit_equal_to_the_no_grad_route_and_reproducible(pooling):
    from vlsa_amd import VlsaNativeError, functional as VF
    k, K = Z.topk_of(pooling), 18
    bags = _gpu_bags("ragged", "bf16")
    T, ls = Z.text_of(K, 11000), torch.tensor(cases.LOGIT_SCALE)
    G = Z.upstream_of(len(bags), K, 11000)
    a, b = _pool(bags, T, ls, k, G), _pool(bags, T, ls, k, G)
    with torch.no_grad():
        plain = VF.zeroshot_pool_bags(bags, T.cuda(), ls.cuda(), k)
    assert torch.equal(a[0], plain)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    bad = [bags[0], bags[1].float().to(torch.bfloat16).requires_grad_(True)]
    with pytest.raises(VlsaNativeError):
        VF.zeroshot_pool_bags(bad, T.cuda().requires_grad_(True), ls.cuda(), k)


class _Prompts(torch.nn.Module):
    """a trainable text side: K raw text features as a parameter (what a CoOp learner + tower hand the model)"""

    def __init__(self, K, seed):
        super().__init__()
        self.t = torch.nn.Parameter(torch.randn(K, 512, generator=cases.gen(seed)))

    def forward(self):
        return self.t * 1.0


def _net(pooling, K=4, seed=77):
    from vlsa_amd.vlsa import VLSA
    return VLSA.from_modules(dict(name="FeatMIL", dim_in=512, pooling=pooling), text_provider=_Prompts(K, seed),
                             logit_scale_init=cases.LOGIT_SCALE).cuda().train()


def _five_bags(dtype=torch.bfloat16):
    return [cases.make_bag(n, 9100 + i, "clustered").to(dtype).cuda() for i, n in enumerate((700, 64, 1, 2798, 333))]


@pytest.mark.parametrize("pooling", ["logit_top10", "logit_mean"])
def test_forward_bags_equals_the_bag_by_bag_calls(pooling):
    bags = _five_bags(torch.float32)
    G = torch.randn(len(bags), 4, generator=cases.gen(5)).cuda()
    res = {}
    for batched in (False, True):
        net = _net(pooling)
        if batched:
            logits, feats, That = net.forward_bags(bags)
            assert feats is None                                             # as the no-grad batched route: only on request
            assert That.requires_grad and logits.grad_fn is not None
        else:
            outs = [net(x[None]) for x in bags]
            logits, That = torch.cat([o[0] for o in outs]), outs[0][2]
        (logits * G).sum().backward()
        res[batched] = (logits.detach(), That.detach(), net.prompt_adapter.t.grad.clone(), net.logit_scale.grad.clone())
    a, b = res[False], res[True]
    assert float((a[0] - b[0]).abs().max()) < 1e-4
    assert float((a[1] - b[1]).abs().max()) < 1e-6
    assert float((a[2] - b[2]).abs().max()) < 1e-4 * float(a[2].abs().max())
    assert float((a[3] - b[3]).abs().max()) < 1e-4 * float(a[3].abs().max())
    net = _net(pooling)
    net.return_patch_features = True
    feats = net.forward_bags(bags)[1]
    assert [tuple(f.shape) for f in feats] == [(x.shape[0], 512) for x in bags]
    assert float((feats[0] - torch.nn.functional.normalize(bags[0], dim=-1)).abs().max()) < 1e-6
    net.return_patch_features = False
    assert net.forward_bags(bags)[1] is None
    # a gradient that arrives through the returned unit text features reaches the prompts too
    net = _net(pooling)
    That = net.forward_bags(bags)[2]
    W = torch.randn(4, 512, generator=cases.gen(6)).cuda()
    (That * W).sum().backward()
    t = net.prompt_adapter.t.detach().clone().requires_grad_(True)
    (torch.nn.functional.normalize(t, dim=-1) * W).sum().backward()
    assert float((net.prompt_adapter.t.grad - t.grad).abs().max()) < 1e-4 * float(t.grad.abs().max())


def _train(mode, pooling, steps=3):
    """mode: 'torch' (the bag-by-bag calls), 'eager' / 'graph' (forward_bags over a BagSet)"""
    from vlsa_amd.functional import BagSet
    from vlsa_amd.losses import SurvObjective
    from vlsa_amd.optim import FusedAdam
    from vlsa_amd.train_step import TrainStep
    net = _net(pooling, K=4, seed=78)
    bags = _five_bags()
    if mode == "torch":
        net.forward_bags = lambda bs: (torch.cat([net(x[None])[0] for x in bs]), None, None)
    named = [net.prompt_adapter.t, net.logit_scale]
    ts = TrainStep(net, SurvObjective(), FusedAdam([{"params": named, "weight_decay": 0.0}], lr=1e-3), graph=mode == "graph")
    t = torch.tensor([0, 2, 1, 2, 0]).cuda()
    e = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0]).cuda()
    bs = BagSet(bags)
    losses = [float(ts.step(bs, t, e)) for _ in range(steps)]
    return losses, [p.detach().clone() for p in named], ts


@pytest.mark.parametrize("pooling", ["logit_top10", "logit_mean"])
def test_train_step_over_a_bag_set_eager_and_captured(pooling):
    lt, pt, _ = _train("torch", pooling)
    le, pe, _ = _train("eager", pooling)
    lg, pg, ts = _train("graph", pooling)
    d = ts.describe()
    assert d["captures"] == 1 and d["replays"] >= 1 and d["why_eager"] is None, d
    for a, b in zip(pt, pe):
        assert float((a - b).abs().max()) < 1e-4 * float(a.abs().max())
    for a, b in zip(lt, le):
        assert abs(a - b) < 1e-4 * max(1.0, abs(a))
    # the replayed step is the eager step: the same kernels in the same order, so a few fp32 ulps at the most (the bound of
    # test_gpu_train_step_graph.py)
    print(f"{pooling}: eager vs replayed: parameters {[float((a - b).abs().max()) for a, b in zip(pe, pg)]}, "
          f"losses {[abs(a - b) for a, b in zip(le, lg)]}")
    for a, b in zip(pe, pg):
        assert float((a - b).abs().max()) <= 2e-6 * max(1.0, float(a.abs().max()))
    for a, b in zip(le, lg):
        assert abs(a - b) <= 2e-6 * max(1.0, abs(a))
