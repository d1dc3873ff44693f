"""The two row groups of the bf16 batched streaming kernel run one barrier apart (vlfan_batch.hip, tile loop): row group 1
enters every bag one barrier late and row group 0 passes one extra barrier after its last tile.  These cases stress the ends
of that stagger: workgroups with an odd number of tiles (row group 1 runs out first), a single tile, no tile at all, bags of
1 / 31 / 33 / 63 / 65 rows, B not a multiple of the number of bags in flight S, 256 slide-sized bags in one launch, and the
scores instantiation (attention weights).  The backward kernels share the forward's row split (vlfan_stream.h): their case
asks for every number of bags in flight directly."""
import pytest
import torch

import cases
from oracle import vlsa_oracle as O

pytestmark = pytest.mark.gpu
P, K, D = 12, 4, 512
TOL = 1e-4
GRAD_RTOL = 1e-4  # relative to the largest gradient entry, as in test_gpu_batch_backward.py (observed <= 2.6e-5: profiles/r04_grad_errors.txt)
# 2960 and 5000 rows leave a last 64-row unit of 16 / 8 rows (one tile: odd tile counts on the workgroups that get it)
SMALL = [1, 31, 33, 63, 65, 2960, 5000]


def _args(params, Q, dev):
    return [t.to(dev) for t in (Q, params["T"], torch.tensor(cases.LOGIT_SCALE), params["W"], params["b"])]


def _oracle(x, Q, params):
    return O.vlsa_vlfan_forward(x.float(), Q, params["T"], torch.tensor(cases.LOGIT_SCALE), head_weight=params["W"],
                                head_bias=params["b"])


@pytest.mark.parametrize("groups", [1, 2, 4])
def test_ragged_small_bags_every_groups_vs_oracle(groups):
    """B = 7 (not a multiple of S = 2 or 4); S = 1 leaves most of the 256 workgroups without rows of a small bag."""
    from vlsa_amd import functional as F
    dev = torch.device("cuda", 0)
    bags = [cases.make_bag(n, 9500 + i, "clustered" if i % 2 else "iid").to(torch.bfloat16) for i, n in enumerate(SMALL)]
    params = cases.make_params(P, K, 9510)
    Q = 0.5 * params["resid"] + params["prompt"]
    plan = F.VlfanBatchPlan(len(bags), P, K, dev)
    plan.set_bags([x.to(dev) for x in bags])
    plan.groups = groups
    for _ in range(2):
        logits = plan.run(*_args(params, Q, dev)).clone()
    torch.cuda.synchronize()
    for i, x in enumerate(bags):
        r = _oracle(x, Q, params)
        assert (logits[i].cpu() - r["logits"][0]).abs().max().item() < TOL, (groups, i, SMALL[i])
        assert (plan.incidence[i].cpu() - r["incidence"][0]).abs().max().item() < TOL, (groups, i, SMALL[i])


# one row, one short of a unit, exactly a unit and one over for the 16-row (fp32) and 32-row (bf16) units of the backward kernels;
# 300 rows = fewer units than workgroups: most of the 512 / S workgroups of the bag own nothing
BWD_SIZES = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300, 1000]


@pytest.mark.parametrize("dtype,nP", [(torch.bfloat16, 12), (torch.float32, 16)])
def test_backward_row_split_every_groups_vs_oracle(dtype, nP):
    """vlsa_vlfan_backward_batch with groups = 1, 2, 4, 8 given directly (the autograd path only ever passes choose_groups'
    pick): dE of every row split against torch autograd through the CPU oracle, and the four against each other."""
    from vlsa_amd import functional as F
    from vlsa_amd import _native as nat
    dev = torch.device("cuda", 0)
    lib, B = nat.load(), len(BWD_SIZES)
    bags = [cases.make_bag(n, 9800 + i, "clustered" if i % 2 else "iid").to(dtype) for i, n in enumerate(BWD_SIZES)]
    params = cases.make_params(nP, K, 9810)
    Q = 0.5 * params["resid"] + params["prompt"]
    dout = torch.randn(B, nP, D, generator=cases.gen(9811))
    # reference: out, (m, l) and dE = d sum(out * dout) / d (unit queries) of the oracle's single-pass restatement
    E = O.l2_normalize(Q).requires_grad_(True)
    outs, ms, ls, total = [], [], [], 0.0
    for x, g in zip(bags, dout):
        m, l, acc, _ = O.vlfan_partial(x.float(), E)
        out = acc / l[:, None]
        total = total + (out * g).sum()
        outs.append(out.detach())
        ms.append(m.detach())
        ls.append(l.detach())
    total.backward()
    ref = E.grad
    scale = ref.abs().max().item()
    m2 = torch.zeros(B, nat.P_STRIDE)
    lsum = torch.ones(B, nat.P_STRIDE)
    m2[:, :nP] = torch.stack(ms) * 1.4426950408889634   # log2 domain
    lsum[:, :nP] = torch.stack(ls)
    m2, lsum, out_d, dout_d = m2.to(dev), lsum.to(dev), torch.stack(outs).to(dev), dout.to(dev)
    table = F._BagTable([x.to(dev) for x in bags])
    qp = F.prepare_queries(Q.to(dev))
    G = lib.vlsa_bwd_batch_partials()
    assert G == 512
    got = {}
    for groups in (1, 2, 4, 8):
        pm = torch.empty(G, nat.P_STRIDE, dtype=torch.float32, device=dev)
        pl = torch.empty(G, nat.P_STRIDE, dtype=torch.float32, device=dev)
        pacc = torch.empty(G, nP, D, dtype=torch.float32, device=dev)
        prep = torch.empty(lib.vlsa_bwd_batch_prep_bytes(B, D), dtype=torch.uint8, device=dev)
        nat.check(lib.vlsa_vlfan_backward_batch(F._p(table.desc), B, table.dt, D, F._p(qp.buf), nP, F.COATTN_SCALE, F._p(dout_d),
                                                F._p(out_d), F._p(m2), F._p(lsum), F._p(prep), F._p(pm), F._p(pl), F._p(pacc),
                                                groups, F._stream()), "vlsa_vlfan_backward_batch")
        got[groups] = F.vlfan_merge(pm, pl, pacc, normalise=False)[2].cpu()
        err = (got[groups] - ref).abs().max().item()
        print(f"groups {groups}: max |dE - ref| = {err:.3e} (largest entry {scale:.3e}, bound {GRAD_RTOL * scale:.3e})")
        assert err < GRAD_RTOL * scale, (groups, err, scale)
    for groups in (2, 4, 8):
        assert (got[groups] - got[1]).abs().max().item() < GRAD_RTOL * scale, groups


@pytest.mark.parametrize("groups", [1, 4])
def test_scores_instantiation_small_bags(groups):
    """want_attn (the kScores instantiation): same logits bit for bit as without scores, A against the oracle."""
    from vlsa_amd import functional as F
    dev = torch.device("cuda", 0)
    bags = [cases.make_bag(n, 9600 + i).to(torch.bfloat16) for i, n in enumerate(SMALL)]
    params = cases.make_params(P, K, 9610)
    Q = 0.5 * params["resid"] + params["prompt"]
    plan = F.VlfanBatchPlan(len(bags), P, K, dev, want_attn=True)
    plan.set_bags([x.to(dev) for x in bags])
    plan.groups = groups
    ref_plan = F.VlfanBatchPlan(len(bags), P, K, dev)
    ref_plan.set_bags([x.to(dev) for x in bags])
    ref_plan.groups = groups
    logits = plan.run(*_args(params, Q, dev)).clone()
    ref_logits = ref_plan.run(*_args(params, Q, dev))
    torch.cuda.synchronize()
    assert torch.equal(logits, ref_logits)
    for i, x in enumerate(bags):
        r = O.vlfan_forward(x.float(), Q)
        A = plan.attn.views[i].cpu()
        assert (A - r["A"]).abs().max().item() < TOL, (groups, i, SMALL[i])


def test_256_slide_sized_bags_vs_single_bag_path():
    """256 bags of 1.5k-6k rows in one launch against the single-bag path (every bag) and the CPU oracle (a sample)."""
    from vlsa_amd import functional as F
    dev = torch.device("cuda", 0)
    sizes = [1500 + (i * 977) % 4500 for i in range(256)]
    bags = [cases.make_bag(n, 9700 + i).to(torch.bfloat16).to(dev) for i, n in enumerate(sizes)]
    params = cases.make_params(P, K, 9710)
    Q = 0.5 * params["resid"] + params["prompt"]
    args = _args(params, Q, dev)
    plan = F.VlfanBatchPlan(len(bags), P, K, dev)
    plan.set_bags(bags)
    logits = plan.run(*args).clone()
    torch.cuda.synchronize()
    for i, n in enumerate(sizes):
        single = F.VlfanInferencePlan(n, D, P, K, dev)
        ref = single.run(bags[i], *args)
        torch.cuda.synchronize()
        assert (logits[i] - ref).abs().max().item() < TOL, (i, n)
    for i in (0, 17, 101, 255):
        r = _oracle(bags[i].cpu(), Q, params)
        assert (logits[i].cpu() - r["logits"][0]).abs().max().item() < TOL, (i, sizes[i])
