"""The two row groups of the bf16 batched streaming kernel run one barrier apart (vlfan_batch.hip, tile loop): row group 1
enters every bag one barrier late and row group 0 passes one extra barrier after its last tile.  These cases stress the ends
of that stagger: workgroups with an odd number of tiles (row group 1 runs out first), a single tile, no tile at all, bags of
1 / 31 / 33 / 63 / 65 rows, B not a multiple of the number of bags in flight S, 256 slide-sized bags in one launch, and the
scores instantiation (attention weights)."""
import pytest
import torch

import cases
from oracle import vlsa_oracle as O

pytestmark = pytest.mark.gpu
P, K, D = 12, 4, 512
TOL = 1e-4
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
