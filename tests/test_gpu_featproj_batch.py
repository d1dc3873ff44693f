"""Feat_Projecter over a batch of bags (Feat_Projecter.forward_bags -> VF.feat_project_bags -> vlsa_feat_project_batch, and under
autograd vlsa_feat_project_rowstats_batch + vlsa_feat_project_backward with B bags): every row against the CPU oracle AND bit for
bit against the per-bag kernel, edge rows in a partial tile, the parameter gradients against torch autograd (and against the per-bag
route's own error), the launch counts, the routes of VLSA.forward_bags, the fallbacks and a TrainStep with a projecter in front."""
import pytest
import torch

import cases

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = 1e-4                      # tests/test_gpu_feat_proj.py


def _params(seed, scale=1.0):
    g = cases.gen(seed)
    u = lambda *s, b: (torch.rand(*s, generator=g) * 2 - 1) * b  # noqa: E731
    return u(512, 512, b=scale / 512 ** 0.5), u(512, b=0.1), 1.0 + u(512, b=0.3), u(512, b=0.2)


def _projecter(seed=5400, scale=2.0, dim=512):
    from vlsa_amd.layers import Feat_Projecter
    m = Feat_Projecter(dim, dim)
    if dim == 512:
        W, b, gm, bt = _params(seed, scale)
        with torch.no_grad():
            m.projecter[0].weight.copy_(W); m.projecter[0].bias.copy_(b)
            m.projecter[1].weight.copy_(gm); m.projecter[1].bias.copy_(bt)
    return m.to(DEV)


def _tcga_sizes():
    return [int(x) for x in torch.randint(2000, 12000, (32,), generator=torch.Generator().manual_seed(0))]


SIZE_LISTS = {
    "one_bag": [777],
    "one_row_bags": [1, 1, 1],
    "tile_heights": [31, 32, 33, 63, 64, 65, 127, 128, 129],
    "tcga_32": None,                                     # bench.py's seed-0 list, filled in below
    "bags_64": [1 + (173 * i) % 700 for i in range(64)],
    "bags_65": [1 + (97 * i) % 500 for i in range(65)],
    "tall_tiles": [9000, 1, 7000, 129],                  # > 120 x 128 rows together: 128-row (bf16) / 64-row (fp32) tiles
}


def _host_bags(sizes, dtype, seed):
    return [cases.make_bag(n, seed + i, "clustered" if i % 2 else "iid").to(dtype) for i, n in enumerate(sizes)]


def _oracle_and_per_bag(m, host, dev_bags):
    """(max |Y_batch - oracle| over the bags, all rows bit-equal to the per-bag kernel) for forward_bags under no_grad"""
    from oracle import vlsa_oracle as O
    lin, norm = m.projecter[0], m.projecter[1]
    P = [t.detach().cpu() for t in (lin.weight, lin.bias, norm.weight, norm.bias)]
    with torch.no_grad():
        got = m.forward_bags(dev_bags)
        per_bag = [m(x) for x in dev_bags]
    torch.cuda.synchronize()
    assert len(got) == len(dev_bags)
    worst = 0.0
    for i, (x, y, y1) in enumerate(zip(host, got, per_bag)):
        assert y.shape == (x.shape[0], 512) and y.dtype == torch.float32
        err = (y.cpu() - O.feat_projecter_forward(x.float(), *P)).abs().max().item()
        worst = max(worst, err)
        assert err < TOL, (i, x.shape[0], err)
        assert torch.equal(y, y1), f"bag {i} ({x.shape[0]} rows): a row differs from the per-bag kernel's"
    return worst


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(SIZE_LISTS))
def test_forward_parity_with_the_oracle_and_bit_equality_with_the_per_bag_kernel(name, dtype):
    sizes = SIZE_LISTS[name] or _tcga_sizes()
    m = _projecter()
    host = _host_bags(sizes, dtype, 6000)
    worst = _oracle_and_per_bag(m, host, [x.to(DEV) for x in host])
    print(f"[featproj batch] {name} {dtype}: {len(sizes)} bags, {sum(sizes)} rows, max |Y - oracle| = {worst:.3e}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_rows_that_are_strided_views_of_a_wider_matrix_and_a_bagset(dtype):
    from vlsa_amd import functional as VF
    sizes = [300, 1, 65, 2798]
    m = _projecter()
    host = _host_bags(sizes, dtype, 6100)
    wide = [torch.zeros(x.shape[0], 640, dtype=dtype, device=DEV) for x in host]
    for w, x in zip(wide, host):
        w[:, :512] = x.to(DEV)
    views = [w[:, :512] for w in wide]
    assert all(v.stride(0) == 640 for v in views)
    _oracle_and_per_bag(m, host, views)
    with torch.no_grad():
        a = m.forward_bags(VF.BagSet(views))                                      # tables derived on the device from the set's descriptor
        b = m.forward_bags(views)
        c = m.forward_bags([x.to(DEV)[None] for x in host])                       # [1, N, 512] bags come back as [1, N, 512]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(y.shape == (1, n, 512) and torch.equal(y[0], x) for x, y, n in zip(b, c, sizes))


def test_edge_rows_in_the_last_partial_tile_of_a_middle_bag():
    """the zero row, the 1e3 row and the 1e-6 row of tests/test_gpu_feat_proj.py::test_constant_and_large_rows, same bounds"""
    from oracle import vlsa_oracle as O
    m = _projecter(5201, scale=1.0)
    with torch.no_grad():
        m.projecter[0].bias.zero_()                   # the zero row projects to exactly 0: variance 0, output = beta
    host = _host_bags([200, 300, 150], torch.float32, 6200)
    X = host[1]                                       # 300 rows: the last 32-row tile holds rows 288..299
    X[290] = 0.0
    X[291] = X[291] * 1e3
    X[292] = X[292] * 1e-6
    with torch.no_grad():
        got = m.forward_bags([x.to(DEV) for x in host])
    P = [t.detach().cpu() for t in (m.projecter[0].weight, m.projecter[0].bias, m.projecter[1].weight, m.projecter[1].bias)]
    for x, y in zip(host, got):
        assert torch.isfinite(y).all()
        assert (y.cpu() - O.feat_projecter_forward(x, *P)).abs().max().item() < 2e-4
    assert (got[1][290].cpu() - P[3]).abs().max().item() < 1e-6


# ---- gradients ------------------------------------------------------------------------------------------------------------------
GRAD_SIZES = [300, 2798, 1, 900, 65, 1500, 33, 640]


def _vlfan(seed=21):
    from vlsa_amd.deepmil import VLFAN
    torch.manual_seed(seed)
    m = VLFAN(dim_in=512, dim_hid=256, use_feat_proj=True, drop_rate=0.0, query="Parameter", num_query=12, query_pooling="mean",
              pred_head="default").to(DEV)
    return m


def _deepmil(seed=22):
    from vlsa_amd.deepmil import DeepMIL
    torch.manual_seed(seed)
    m = DeepMIL(dim_in=512, dim_hid=256, num_cls=5, use_feat_proj=True, drop_rate=0.0, pooling="gated_attention", pred_head="default").to(DEV)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("bias"):
                p.add_(0.05 * torch.randn_like(p))
    return m


def _torch_vlfan(m, leaves, bags):
    from oracle import vlsa_oracle as O
    fp = tuple(leaves["feat_proj.projecter." + k] for k in ("0.weight", "0.bias", "1.weight", "1.bias"))
    return torch.stack([O.vlfan_forward(x.float(), leaves["Q"], head_weight=leaves["visual_adapter.weight"],
                                        head_bias=leaves["visual_adapter.bias"], scale=m.coattn_scale(), feat_proj=fp)["v"] for x in bags])


def _torch_deepmil(m, leaves, bags):
    from oracle import vlsa_oracle as O
    import torch.nn.functional as F
    fp = tuple(leaves["feat_proj.projecter." + k] for k in ("0.weight", "0.bias", "1.weight", "1.bias"))
    s = "sigma."
    rows = []
    for x in bags:
        y = O.feat_projecter_forward(x.float(), *fp)
        pooled, _, _ = O.gated_attention_pooling(y, leaves[s + "fc1.0.weight"], leaves[s + "fc1.0.bias"], leaves[s + "score.0.weight"],
                                                 leaves[s + "score.0.bias"], leaves[s + "fc2.weight"], leaves[s + "fc2.bias"])
        rows.append(pooled)
    f = torch.stack(rows)
    return F.linear(f, leaves["g.weight"], leaves["g.bias"]) if "g.weight" in leaves else f


def _grads_of(m, out, G):
    (out * G).sum().backward()
    g = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return g


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("enc", ["vlfan", "deepmil"])
def test_gradients_against_torch_autograd_and_the_per_bag_route(enc, dtype):
    """dW, db, dgamma, dbeta of the projecter and the query / pooling gradients of the module behind it, 8 ragged bags: the batched
    route against torch autograd over a plain fp32 restatement (oracle/vlsa_oracle.py on the device); bounds: 2e-3 x max|ref| for the
    projecter weight (tests/test_gpu_feat_proj.py), 1e-4 x max|ref| for the rest with the floor and the scale for the score
    layer's output bias that tests/test_gpu_deepmil_train_batch.py::_close uses (its gradient is exactly zero for a softmax
    pooling: both sides return cancellation noise).  And for these tensors -- the projecter's, the queries, the pooling module's --
    the batched route's error is at most twice the per-bag route's.  The head behind the encoder (visual_adapter / g) is checked
    against the bounds only: it never sees the projecter, and its bias gradient is a plain sum of the upstream rows that the per-bag
    route accumulates in the very order of the torch reference (error exactly 0 there, one fp32 ulp for a batched Linear)."""
    m = (_vlfan() if enc == "vlfan" else _deepmil()).eval()          # (dropout 0 anyway)
    bags = [x.to(DEV) for x in _host_bags(GRAD_SIZES, dtype, 6300)]
    named = dict(m.named_parameters())
    leaves = {n: p.detach().clone().requires_grad_(True) for n, p in named.items()}
    ref_out = (_torch_vlfan if enc == "vlfan" else _torch_deepmil)(m, leaves, bags)
    G = torch.randn(ref_out.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    (ref_out * G).sum().backward()
    ref = {n: leaf.grad for n, leaf in leaves.items() if leaf.grad is not None}
    got_out = m.forward_bags(bags)
    batched = _grads_of(m, got_out, G)
    per_bag = _grads_of(m, torch.cat([m(x[None]) for x in bags]), G)
    assert (got_out - ref_out).abs().max().item() < TOL * max(1.0, ref_out.abs().max().item())
    assert set(batched) == set(ref) == set(per_bag), (sorted(batched), sorted(ref))
    assert "feat_proj.projecter.0.weight" in batched
    big = max(g.abs().max().item() for g in ref.values())
    failures = []
    for n in sorted(ref):
        r = ref[n]
        eb = (batched[n] - r).abs().max().item()
        ep = (per_bag[n] - r).abs().max().item()
        is_c = n.endswith("sigma.fc2.bias")
        rel = 2e-3 if n == "feat_proj.projecter.0.weight" else 1e-4
        tol = rel * max(big if is_c else r.abs().max().item(), 1e-2)
        cases.record_grad_error(f"{enc} batched {n}", eb, r.abs().max().item(), tol)
        cases.record_grad_error(f"{enc} per-bag {n}", ep, r.abs().max().item(), tol)
        print(f"[featproj batch grad] {enc} {dtype} {n}: batched {eb:.3e} per-bag {ep:.3e} tol {tol:.3e} max|ref| {r.abs().max().item():.3e}")
        if eb > tol:
            failures.append(f"{n}: batched error {eb:.3e} > {tol:.3e}")
        if (n.startswith("feat_proj.") or n == "Q" or n.startswith("sigma.")) and eb > 2 * ep:
            failures.append(f"{n}: batched error {eb:.3e} > 2 x per-bag error {ep:.3e}")
    assert not failures, failures


# ---- one launch -------------------------------------------------------------------------------------------------------------------
def _count(monkeypatch, names):
    from vlsa_amd import _native
    lib = _native.load()
    counts = {n: 0 for n in names}
    for n in names:
        fn = getattr(lib, n)

        def wrapped(*a, _fn=fn, _n=n):
            counts[_n] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, n, wrapped)
    return counts


PER_BAG = ("vlsa_feat_project", "vlsa_feat_project_train", "vlsa_feat_project_rowstats")
BATCH = ("vlsa_feat_project_batch", "vlsa_feat_project_rowstats_batch", "vlsa_feat_project_backward")


@pytest.mark.parametrize("B", [32, 65])
def test_a_chunk_of_bags_is_one_launch_each_way(B, monkeypatch):
    m = _projecter()
    sizes = [40 + (61 * i) % 900 for i in range(B)]
    bags = [x.to(DEV) for x in _host_bags(sizes, torch.bfloat16, 6400)]
    chunks = (B + 63) // 64
    counts = _count(monkeypatch, PER_BAG + BATCH)
    with torch.no_grad():
        m.forward_bags(bags)
    assert [counts[n] for n in PER_BAG] == [0, 0, 0], counts
    assert counts["vlsa_feat_project_batch"] == chunks and counts["vlsa_feat_project_backward"] == 0, counts
    ys = m.forward_bags(bags)                                  # training forward + backward
    assert all(y.requires_grad for y in ys)
    sum((y * y).sum() for y in ys).backward()
    torch.cuda.synchronize()
    assert [counts[n] for n in PER_BAG] == [0, 0, 0], counts
    assert counts["vlsa_feat_project_batch"] == 2 * chunks, counts
    assert counts["vlsa_feat_project_rowstats_batch"] == chunks and counts["vlsa_feat_project_backward"] == chunks, counts
    assert m.projecter[0].weight.grad is not None and torch.isfinite(m.projecter[0].weight.grad).all()


# ---- routes -------------------------------------------------------------------------------------------------------------------------
def _vlsa(kind, drop=0.0):
    from vlsa_amd.vlsa import VLSA
    if kind == "deepmil":
        cfg = dict(name="DeepMIL", dim_in=512, dim_hid=256, num_cls=512, use_feat_proj=True, drop_rate=drop, pooling="gated_attention",
                   pred_head="default")
    else:
        cfg = dict(name="VLFAN", dim_in=512, dim_hid=256, use_feat_proj=True, drop_rate=drop, num_query=12, query="Parameter",
                   gated_query=False, query_pooling="mean" if kind == "vlfan_mean" else "gated_attention", pred_head="default")
    torch.manual_seed(11)
    return VLSA.from_modules(cfg, pretrained_text_features=torch.randn(4, 512), logit_scale_init=cases.LOGIT_SCALE).to(DEV)


def _same_attn(a, b):
    if isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b)
        for x, y in zip(a, b):
            _same_attn(x, y)
    else:
        assert a.shape == b.shape and (a - b).abs().max().item() < 1e-4


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("kind", ["vlfan_mean", "vlfan_gated_pool", "deepmil"])
def test_vlsa_forward_bags_with_a_projecter_equals_the_per_bag_forward(kind, training, monkeypatch):
    net = _vlsa(kind).train(training)
    bags = [x.to(DEV) for x in _host_bags([300, 2798, 1, 900, 129], torch.bfloat16, 6500)]
    counts = _count(monkeypatch, PER_BAG + BATCH)

    def run():
        got = net.forward_bags(bags)[0]
        assert counts["vlsa_feat_project_batch"] >= 1 and [counts[n] for n in PER_BAG] == [0, 0, 0], counts
        ref = torch.cat([net(x[None])[0] for x in bags])
        assert got.shape == ref.shape and (got - ref).abs().max().item() < 1e-4
        out = net.forward_bags(bags, ret_with_attn=True)
        assert (out[0] - ref).abs().max().item() < 1e-4
        for x, a in zip(bags, out[-1]):
            _same_attn(a, net.mil_encoder(x[None], ret_with_attn=True)[1])
    if training:
        run()
    else:
        with torch.no_grad():
            run()


# ---- fallbacks ----------------------------------------------------------------------------------------------------------------------
def test_what_the_batch_kernel_does_not_take_goes_bag_by_bag(monkeypatch):
    m = _projecter()
    bags = [x.to(DEV) for x in _host_bags([50, 300, 7], torch.float32, 6600)]
    counts = _count(monkeypatch, PER_BAG + BATCH)
    # a bag that requires grad: torch modules, the gradient reaches the bag
    xs = [bags[0], bags[1].clone().requires_grad_(True), bags[2]]
    ys = m.forward_bags(xs)
    assert counts["vlsa_feat_project_batch"] == 0
    for x, y in zip(xs, ys):
        assert torch.equal(y, m(x))
    ys[1].sum().backward()
    assert xs[1].grad is not None and xs[1].grad.shape == xs[1].shape
    # mixed dtypes, an empty bag
    with torch.no_grad():
        mixed = [bags[0], bags[1].to(torch.bfloat16)]
        for x, y in zip(mixed, m.forward_bags(mixed)):
            assert torch.equal(y, m(x))
        empty = [bags[0], bags[1][:0]]
        out = m.forward_bags(empty)
        assert out[1].shape == (0, 512) and torch.equal(out[0], m(bags[0]))
    assert counts["vlsa_feat_project_batch"] == 0
    # a 1024-wide projecter
    m2 = _projecter(dim=1024)
    wide = [torch.randn(n, 1024, generator=cases.gen(n)).to(DEV) for n in (20, 33)]
    with torch.no_grad():
        for x, y in zip(wide, m2.forward_bags(wide)):
            assert y.shape == x.shape and torch.equal(y, m2(x))
    # CPU bags and a CPU module
    mc = _projecter().cpu()
    cpu = [x.cpu() for x in bags]
    with torch.no_grad():
        for x, y in zip(cpu, mc.forward_bags(cpu)):
            assert not y.is_cuda and torch.equal(y, mc(x))
    assert counts["vlsa_feat_project_batch"] == 0


# ---- capture ------------------------------------------------------------------------------------------------------------------------
def _steps(net, graph, n, bags, t, e, toggle_after=()):
    from vlsa_amd.losses import SurvObjective
    from vlsa_amd.optim import FusedAdam
    from vlsa_amd.train_step import TrainStep
    ps = [p for p in net.parameters() if p.requires_grad]
    ts = TrainStep(net, SurvObjective(), FusedAdam([{"params": ps, "weight_decay": 0.0}], lr=1e-3), graph=graph)
    losses = []
    for i in range(n):
        losses.append(float(ts.step(bags, t, e)))
        if i in toggle_after:                      # an eval() pass between two steps: the projecter's cached packed block is re-used
            net.eval()
            with torch.no_grad():
                net.forward_bags(bags)
            net.train()
    return losses, [p.detach().clone() for p in net.parameters()], ts


@pytest.mark.parametrize("frozen", [False, True], ids=["trainable_projecter", "frozen_projecter"])
def test_train_step_with_a_projecter_replays_the_eager_steps(frozen):
    """DeepMIL behind a trainable / a frozen projecter: the same six steps from the same start through TrainStep(graph=False) and
    TrainStep(graph=True) -- three eager steps (two plain, one on the capture stream), then the capture and its replays, an eval()
    pass between two replays -- give the same losses and parameters.  The projecter packs its weights inside the capture and reads
    its tables from the BagSet's descriptor, so the step IS captured."""
    from vlsa_amd import functional as VF
    bags = VF.BagSet([x.to(DEV) for x in _host_bags([300 + 211 * i for i in range(8)], torch.bfloat16, 6700)])
    t = torch.tensor([0, 1, 2, 3, 0, 1, 2, 0], device=DEV)
    e = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 0.0, 1.0], device=DEV)
    nets = [_vlsa("deepmil").train(), _vlsa("deepmil").train()]
    if frozen:
        for net in nets:
            for p in net.mil_encoder.feat_proj.parameters():
                p.requires_grad_(False)
    le, pe, _ = _steps(nets[0], False, 6, bags, t, e, toggle_after=(3,))
    lg, pg, ts = _steps(nets[1], True, 6, bags, t, e, toggle_after=(3,))
    d = ts.describe()
    print(f"[featproj batch capture] frozen={frozen}: {d}; eager {le}; graph {lg}")
    assert d["captures"] == 1 and d["replays"] >= 3 and d["why_eager"] is None, d
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (le, lg)
    for a, b in zip(pe, pg):
        assert (a - b).abs().max().item() <= 1e-6 * max(1.0, a.abs().max().item())
