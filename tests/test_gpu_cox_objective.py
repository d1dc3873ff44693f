"""The continuous survival heads' objective on the device (vlsa_amd/csrc/surv_pairs.hip: SurvPLE, rank_loss, recon_loss, MSE_loss in one
launch) at every batch size the launch branches on, against the float64 restatement of tests/cox_cases.py (which
tests/test_cox_cases_cpu.py pins to the reference's own float64 results).  The gates are 8 x what a plain fp32 evaluation of the same
formulas reaches, measured there; every comparison prints its measured error next to the gate."""
import ctypes

import pytest
import torch

import cox_cases as C

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
_FIELDS = ("ple", "rank", "recon", "mse")


def _dev(*tensors):
    return tuple(x.to(DEV) for x in tensors)


def _bits(x):
    return x.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _objective(c):
    from vlsa_amd.losses import SurvPairObjective
    return SurvPairObjective(**C.spec(c))


def _check(name, c, pred, t, e, want):
    """value, per-term values and gradient of the one launch against the float64 truth `want`; then the autograd route"""
    from vlsa_amd import _native as nat
    from vlsa_amd.losses import PAIR_TERMS
    obj = _objective(c)
    B = pred.numel()
    v, g = obj.value_and_grad(pred, t, e)
    words = obj.terms.cpu()
    ev, eg = C.rel_value(v.cpu(), want.objective), C.rel_grad(g.cpu().reshape(-1), want.grad, B)
    print(f"{name}: objective {v.item():.9g} truth {float(want.objective):.9g} rel {ev:.2e} (gate {C.VALUE_RTOL:g}); gradient rel to "
          f"max(max|truth| = {float(want.grad.abs().max()):.3e}, 1/B): {eg:.2e} (gate {C.GRAD_RTOL:g})")
    assert v.shape == () and g.shape == pred.shape and bool(torch.isfinite(g).all())
    assert ev <= C.VALUE_RTOL and eg <= C.GRAD_RTOL
    computed = C.terms_with_weight(c)
    for field, word in zip(_FIELDS, PAIR_TERMS.values()):
        got = float(words[word])
        if computed[field]:
            et = C.rel_value(got, getattr(want, field))
            print(f"{name}: {field} {got:.9g} truth {float(getattr(want, field)):.9g} rel {et:.2e}")
            assert et <= C.VALUE_RTOL
        else:
            assert got == 0.0
    if computed["rank"]:
        assert int(words[nat.PAIR_OBJ_PAIRS]) == want.pairs          # an integer, exactly
    x = pred.clone().requires_grad_(True)
    (3.0 * obj(x, torch.stack([t, e], dim=1))).backward()                  # the handler's [B, 2] label; the incoming gradient scales
    assert C.rel_grad(x.grad.cpu().reshape(-1), 3.0 * want.grad, B / 3.0) <= C.GRAD_RTOL
    return v, g


# ---- 1. the launch against the float64 truth
@pytest.mark.parametrize("c", C.CASES, ids=C.ids(C.CASES))
def test_objective_against_float64(c):
    i, want = C.case_inputs(c), C.case_truth(c)
    pred, t, e = _dev(i.pred, i.t, i.e)
    v, g = _check(c.name, c, pred, t, e, want)
    if c.censor == "all-censored":          # no event, no pair: +0 (the reference's SurvPLE: -0) and no gradient from either term
        assert float(want.ple) == 0.0 and want.pairs == 0
    if c.censor == "no-pair":
        assert want.pairs == 0 and float(want.rank) == 0.0


@pytest.mark.parametrize("c", C.FIXTURES, ids=C.ids(C.FIXTURES))
def test_objective_against_the_references_float64_results(c):
    fx = C.load_fixture(c)
    pred, t, e = _dev(torch.from_numpy(fx["pred"]), torch.from_numpy(fx["t"]), torch.from_numpy(fx["e"]))
    obj = _objective(c)
    x = pred.view(-1, 1).clone().requires_grad_(True)                    # the [B, 1] head, as calc_objective_loss receives it
    got = obj(x, t.view(-1, 1), e.view(-1, 1))
    got.backward()
    ev = C.rel_value(got.detach().cpu(), fx["ref64_total"])
    eg = C.rel_grad(x.grad.cpu().reshape(-1), torch.from_numpy(fx["ref64_grad"]), c.B)
    print(f"{c.name}: value {ev:.2e} (gate {C.VALUE_RTOL:g}) gradient {eg:.2e} (gate {C.GRAD_RTOL:g})")
    assert x.grad.shape == x.shape and ev <= C.VALUE_RTOL and eg <= C.GRAD_RTOL
    obj.value_and_grad(pred, t, e)
    words = obj.terms.cpu()
    for k, key in enumerate(("ref64_ple", "ref64_rank", "ref64_recon", "ref64_mse")):
        assert C.rel_value(float(words[1 + k]), fx[key]) <= C.VALUE_RTOL, key
    assert int(words[5]) == int(fx["rank_pairs"])


# ---- 2. exact kinks: torch's abs and relu have derivative 0 at 0
@pytest.mark.parametrize("l2", [False, True], ids=["l1", "l2"])
@pytest.mark.parametrize("name", list(C.EDGES))
def test_edges_against_float64(name, l2):
    pred, t, e = _dev(*C.EDGES[name])
    c = C.EDGE_CASE_L2 if l2 else C.EDGE_CASE
    v, g = _check(f"{name}-{'l2' if l2 else 'l1'}", c, pred, t, e, C.edge_truth(name, l2))
    if name == "all-above-the-cap":
        from vlsa_amd.losses import SurvPLE
        x = pred.clone().requires_grad_(True)
        SurvPLE()(x, t, e).backward()
        assert not bool(x.grad.any())


def test_the_cap_itself_still_has_a_gradient():
    """pred == 10.0 exactly: torch.where(y > 10, 10, y) passes the gradient on; 10.000001 does not"""
    from vlsa_amd.losses import SurvPLE
    pred = torch.tensor([10.0, 10.000001, 3.0], device=DEV, requires_grad=True)
    t, e = torch.tensor([1.0, 2.0, 3.0], device=DEV), torch.ones(3, device=DEV)
    SurvPLE()(pred, t, e).backward()
    assert pred.grad[0].item() != 0.0 and pred.grad[1].item() == 0.0 and pred.grad[2].item() != 0.0


# ---- 3. shapes and dtypes of the inputs
@pytest.mark.parametrize("c", [c for c in C.GRID if c.B in (3, 130, 1025)], ids=lambda c: c.name)
def test_column_input_and_float64_times_give_the_same_bits(c):
    i = C.case_inputs(c)
    pred, t, e = _dev(i.pred, i.t, i.e)
    obj = _objective(c)
    v, g = obj.value_and_grad(pred, t, e)
    v2, g2 = obj.value_and_grad(pred.view(-1, 1), t.view(-1, 1), e.view(-1, 1))
    assert g2.shape == (c.B, 1) and _same_bits(v, v2) and _same_bits(g, g2.view(-1))
    v3, g3 = obj.value_and_grad(pred, t.double(), e)               # fp32 times are compared as float64 either way
    assert _same_bits(v, v3) and _same_bits(g, g3)
    v4, g4 = obj.value_and_grad(pred, torch.stack([t, e], dim=1))
    assert _same_bits(v, v4) and _same_bits(g, g4)


def test_float64_times_are_compared_in_float64():
    """two times that differ below fp32's resolution: a rank pair and a smaller risk set under float64, a tie under fp32"""
    from vlsa_amd.losses import SurvPLE, rank_loss
    t64 = torch.tensor([1.0, 1.0 + 2.0 ** -40], dtype=torch.float64, device=DEV)
    pred, e = torch.tensor([0.5, -0.25], device=DEV), torch.ones(2, device=DEV)
    c = C.EDGE_CASE
    for t in (t64, t64.float()):
        want = C.truth(pred.cpu(), t.cpu().double(), e.cpu(), c)
        assert want.pairs == (1 if t.dtype == torch.float64 else 0)
        assert C.rel_value(rank_loss(pred, t, e).cpu(), want.rank) <= C.VALUE_RTOL
        assert C.rel_value(SurvPLE()(pred, t, e).cpu(), want.ple) <= C.VALUE_RTOL


# ---- 4. each module alone is the objective with that one weight, bit for bit; the launch is bit-reproducible
@pytest.mark.parametrize("c", [c for c in C.OPTIONS if c.times == "ties" and sum(w != 0 for w in (c.w_ple, c.w_rank, c.w_recon, c.w_mse)) == 1],
                         ids=lambda c: c.name)
def test_each_module_alone_equals_the_objective_with_that_weight(c):
    from vlsa_amd import losses as L
    i = C.case_inputs(c)
    pred, t, e = _dev(i.pred, i.t, i.e)
    v, g = _objective(c).value_and_grad(pred, t, e)
    x = pred.clone().requires_grad_(True)
    if c.w_ple:
        got = L.SurvPLE()(x, t, e)
    elif c.w_rank:
        got = L.rank_loss(x, t, e, gamma=c.rank_gamma, norm=c.rank_norm)
    elif c.w_recon:
        got = L.recon_loss(x, t, e, alpha=0.9, gamma=c.recon_gamma, norm=c.recon_norm, cur_alpha=c.recon_alpha)     # cur_alpha wins
    else:
        got = L.MSE_loss(x, t, e, include_censored=c.mse_censored)
    got.backward()
    assert got.shape == () and _same_bits(got, v) and _same_bits(x.grad, g)


def test_rank_loss_without_a_pair_is_a_zero_in_the_graph():
    from vlsa_amd.losses import rank_loss
    x = torch.randn(7, device=DEV, requires_grad=True)
    got = rank_loss(x, torch.arange(7.0, device=DEV), torch.zeros(7, device=DEV))
    got.backward()
    assert got.shape == () and got.item() == 0.0 and got.requires_grad and not bool(x.grad.any())
    with pytest.raises(NotImplementedError):
        rank_loss(x, torch.arange(7.0, device=DEV), torch.zeros(7, device=DEV), add_weight=True)


@pytest.mark.parametrize("c", [c for c in C.GRID if c.B in (65, 1025, C.MAX_B) and c.times == "ties"], ids=lambda c: c.name)
def test_two_launches_give_the_same_bits(c):
    i = C.case_inputs(c)
    pred, t, e = _dev(i.pred, i.t, i.e)
    obj = _objective(c)
    v, g = obj.value_and_grad(pred, t, e)
    words = obj.terms.clone()
    for _ in range(2):
        v2, g2 = obj.value_and_grad(pred, t, e)
        assert _same_bits(v, v2) and _same_bits(g, g2) and _same_bits(words, obj.terms)


@pytest.mark.parametrize("c", C.SPLIT_ROUTE, ids=C.ids(C.SPLIT_ROUTE))
def test_4097_samples_take_the_split_route_and_meet_the_same_gates(c):
    from vlsa_amd import losses as L
    i, want = C.case_inputs(c), C.case_truth(c)
    pred, t, e = _dev(i.pred, i.t, i.e)
    assert c.B == C.REFUSED_B and L._pair_route(pred) is L._launch_pair_split and L._pair_route(pred[:C.MAX_B]) is L._launch_pair
    _check(c.name, c, pred, t, e, want)
    _check(c.name + "-column", c, pred.view(-1, 1), t.view(-1, 1), e.view(-1, 1), want)


# ---- 5. graph capture: the launch reads no host data
def _graph_edges(raw_graph):
    """(number of nodes, [(from, to)]) of a captured graph, asked of the HIP runtime this process has loaded"""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    graph, n, m = ctypes.c_void_p(raw_graph), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    assert hip.hipGraphGetEdges(graph, None, None, ctypes.byref(m)) == 0
    src, dst = (ctypes.c_void_p * max(m.value, 1))(), (ctypes.c_void_p * max(m.value, 1))()
    if m.value:
        assert hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(m)) == 0
    return n.value, [(src[k], dst[k]) for k in range(m.value)]


def test_the_launch_replays_from_a_graph_as_a_single_chain():
    c = next(c for c in C.GRID if c.B == 130 and c.times == "ties")
    obj = _objective(c)
    ins = [C.case_inputs(c._replace(seed=c.seed + k)) for k in range(3)]
    pred, t, e = (x.clone() for x in _dev(ins[0].pred, ins[0].t, ins[0].e))
    eager = []
    for i in ins:
        v, g = obj.value_and_grad(*_dev(i.pred, i.t, i.e))
        eager.append((v.clone(), g.clone()))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, stream=s):
        v, g = obj.value_and_grad(pred, t, e)
    for k in (1, 2):
        pred.copy_(ins[k].pred); t.copy_(ins[k].t); e.copy_(ins[k].e)
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(v, eager[k][0]) and _same_bits(g, eager[k][1])
    nodes, edges = _graph_edges(graph.raw_cuda_graph())
    print(f"captured graph: {nodes} node(s), {len(edges)} edge(s)")
    assert nodes >= 1 and len(edges) == nodes - 1                        # a chain ...
    for n in {a for a, _ in edges} | {b for _, b in edges}:              # ... with no fork and no join
        assert sum(a == n for a, _ in edges) <= 1 and sum(b == n for _, b in edges) <= 1


# ---- 6. refusals come from the host checks: nothing is launched
def test_bad_arguments_are_refused_before_any_launch():
    from vlsa_amd import _native as nat
    from vlsa_amd.functional import _p, _stream
    from vlsa_amd.losses import SurvPairObjective
    lib = nat.load()
    B = C.REFUSED_B
    pred, t, e = torch.zeros(B, device=DEV), torch.arange(float(B), device=DEV), torch.ones(B, device=DEV)
    out = torch.full((nat.PAIR_OBJ_WORDS + B,), -7.0, device=DEV)

    def call(pred=pred, t=t, dtype=nat.PAIR_TIME_F32, e=e, B=4, rank_norm=nat.PAIR_NORM_L1, recon_norm=nat.PAIR_NORM_L2, obj=out):
        return lib.vlsa_surv_pair_objective(_p(pred), _p(t), dtype, _p(e), B, 1.0, 1.0, 1.0, 1.0, 1.0, rank_norm, 0.0, 1.0, recon_norm, 0,
                                            _p(obj), _p(out[nat.PAIR_OBJ_WORDS:]), _stream())

    assert call(pred=None) == nat.EINVAL and call(t=None) == nat.EINVAL and call(e=None) == nat.EINVAL and call(obj=None) == nat.EINVAL
    assert call(B=0) == nat.EINVAL and call(B=-1) == nat.EINVAL and call(dtype=2) == nat.EINVAL
    assert call(rank_norm=0) == nat.EINVAL and call(recon_norm=3) == nat.EINVAL
    assert call(B=B) == nat.EUNSUPPORTED and nat.PAIR_MAX_B == C.MAX_B == B - 1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                   # no kernel wrote
    assert call() == nat.OK
    torch.cuda.synchronize()
    assert bool((out[:nat.PAIR_OBJ_WORDS + 4] != -7.0).all()) and bool((out[nat.PAIR_OBJ_WORDS + 4:] == -7.0).all())
    with pytest.raises(nat.VlsaNativeError):                           # no CPU route
        SurvPairObjective(weight_ple=1.0)(pred[:4].cpu(), t[:4].cpu(), e[:4].cpu())


# ---- 7. the [B, 1] head, the objective and the existing backward meet
def test_abmil_head_trains_under_survple():
    from vlsa_amd.losses import SurvPairObjective
    from vlsa_amd.model_utils import load_model
    torch.manual_seed(11)
    net = load_model("DeepMIL", [512, 256, 1], network="ABMIL").to(DEV)
    g = torch.Generator()
    g.manual_seed(12)
    sizes = [300, 17, 129, 64, 257, 1, 200, 96]
    bags = [torch.randn(n, 512, generator=g).to(torch.bfloat16).to(DEV) for n in sizes]
    t = (torch.rand(8, generator=g) * 12.0).to(DEV)
    e = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0], device=DEV)
    pred = net.forward_bags(bags)
    assert pred.shape == (8, 1)
    value, grad = SurvPairObjective(weight_ple=1.0).value_and_grad(pred, t, e)
    want = C.truth(pred.detach().cpu(), t.cpu(), e.cpu(), C.EDGE_CASE._replace(w_rank=0.0, w_recon=0.0, w_mse=0.0))
    assert grad.shape == pred.shape and C.rel_value(value.cpu(), want.objective) <= C.VALUE_RTOL
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    pred.backward(grad, retain_graph=True)
    got = [p.grad.clone() for _, p in named]
    for _, p in named:
        p.grad = None
    pred.backward(want.grad.to(device=DEV, dtype=pred.dtype).view_as(pred))
    for (name, p), a in zip(named, got):
        scale = float(p.grad.abs().max())
        err = float((a - p.grad).abs().max())
        print(f"{name}: max|grad| {scale:.3e}, difference between the two seeds {err:.2e} (gate {C.GRAD_RTOL:g} x scale)")
        assert scale > 0 and err <= C.GRAD_RTOL * scale
