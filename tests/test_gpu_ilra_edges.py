"""ILRA's kernels (vlsa_amd/csrc/ilra.hip) at every instantiation, cap, stride and peak: the table of ilra_edge_cases.py replayed on
the GPU against the float64 formulas of ilra_helpers.py (the row map with the KERNEL's ReLU decisions, its mask within the case's band),
and the module against ``run64`` where a branch is reached through it only.  Packed rows without a gradient, bag rows behind a row
stride of 1024, fp32 bags in ragged tables, 1 .. 16 queries, both sides of the part and the split cap, score profiles that lift the
running maximum on every tile or underflow whole parts, 64 bags per chunk and bags shorter than the column sums' eight segments.
Gate everywhere: ``ilra_helpers.TOL`` by ``rel`` / ``check_grads``.  Every comparison prints its figure before it asserts."""
import re

import numpy as np
import pytest
import torch

import ilra_cases as IC
import ilra_edge_cases as EC
import ilra_helpers as IH

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = IH.TOL


_run, _check, _run_module, _check_module = IH.run_case, IH.check_case, IH.run_module, IH.check_module


def _replay(name):
    case = EC.BY_NAME[name]
    inp = EC.make_inputs(case)
    got = _run(case, inp)
    _check(case, inp, got)
    return case, inp, got


def _same_bits(tag, a, b, keys):
    for k in keys:
        same = torch.equal(a[k], b[k])
        print(f"[ilra {tag}] {k}: {'bit-identical' if same else 'DIFFERS by %.2e' % float((a[k].double() - b[k].double()).abs().max())}")
        assert same, (tag, k)


# ---- 1. packed rows without a gradient ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.names("nograd"))
def test_packed_rows_without_a_gradient(name):
    """k_ip_backward<float, 256, false> / k_rm_backward<float, 256, false>: against float64, and the same bits as with a gradient on
    the rows -- the DX branch only adds work behind the chains both share"""
    case, inp, plain = _replay(name)
    assert plain["dX"] is None
    full = _run(case, inp, xgrad=True)
    _check(case._replace(xgrad=True), inp, full)
    _same_bits(name + " plain xp vs xp.requires_grad_()", plain, full,
               ["Z", "dE"] if case.kind == "pool" else ["xhat", "mask"] + ["d" + k for k in IH.ROWMAP_KEYS])


def test_first_block_frozen():
    """gab_blocks.0 frozen: the second block's and the pooling's packed rows carry no gradient.  The remaining gradients against run64,
    and bit for bit those of the all-trainable model"""
    L, w = 2, IC.make_w(4, 931)
    x, params = IC.make_bag(130, "bf16", 931), IC.make_params(L, 4, 931)
    m = IH.build_model(L, 4, params, DEV)
    bags = [IH.bag(x, "bf16", DEV)]
    _, _, g_all = _run_module(m, bags, w)
    for p in m.gab_blocks[0].parameters():
        p.requires_grad_(False)
    logits, states, grads = _run_module(m, bags, w)
    assert grads and not any(k.startswith("gab_blocks.0.") for k in grads) and all(p.grad is None for p in m.gab_blocks[0].parameters())
    assert set(grads) == {k for k in params if not k.startswith("gab_blocks.0.")}
    _check_module("block 0 frozen", logits, states, grads, [x], params, L, w)
    _same_bits("block 0 frozen vs all trainable", grads, g_all, sorted(grads))


# ---- 2. a row stride other than D -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.names("strided"))
def test_strided_bag_alone(name):
    case, inp, got = _replay(name)
    flat = _run(case, inp, stride=512)
    _same_bits(name + " stride 1024 vs contiguous", got, flat, [k for k, v in got.items() if v is not None])


@pytest.mark.parametrize("rows", ["bf16", "f32"])
@pytest.mark.parametrize("N", [17, 300])
def test_strided_bag_through_the_module(N, rows):
    L, seed = 2, 940 + N
    x, params, w = IC.make_bag(N, rows, seed), IC.make_params(L, 4, seed), IC.make_w(4, seed)
    m = IH.build_model(L, 4, params, DEV)
    flat = IH.bag(x, rows, DEV)
    arena = torch.full((N, 1024), float("nan"), dtype=flat.dtype, device=DEV)
    arena[:, :512] = flat
    view = arena[:, :512]
    assert view.stride(0) == 1024
    logits, states, grads = _run_module(m, [view], w)
    _check_module(f"strided module N={N} {rows}", logits, states, grads, [x], params, L, w)
    l2, _, g2 = _run_module(m, [flat], w)
    _same_bits(f"strided module N={N} {rows} vs contiguous", {**grads, "logits": logits}, {**g2, "logits": l2}, ["logits"] + sorted(grads))


# ---- 3. fp32 bags in a batch ----------------------------------------------------------------------------------------------------------
F32_BATCH = [1, 17, 130, 300, 64]


def test_fp32_batch_equals_single_calls_and_float64_and_is_reproducible():
    L = 2
    params = IC.make_params(L, 4, 950)
    m = IH.build_model(L, 4, params, DEV)
    xs = [IC.make_bag(n, "f32", 951 + i) for i, n in enumerate(F32_BATCH)]
    bags = [IH.bag(x, "f32", DEV) for x in xs]
    w = np.random.RandomState(952).standard_normal((len(xs), 4)).astype(np.float32)
    logits, states, grads = _run_module(m, bags, w)
    singles, gsum = [], None
    for i, x in enumerate(bags):
        out, _, g = _run_module(m, [x], w[i:i + 1])
        singles.append(out)
        gsum = {k: v.double() for k, v in g.items()} if gsum is None else {k: gsum[k] + g[k].double() for k in g}
    same = torch.equal(logits, torch.cat(singles))
    print(f"[ilra fp32 batch] logits vs single calls: {'bit-identical' if same else float((logits - torch.cat(singles)).abs().max())}")
    assert same
    IH.check_grads("fp32 batch vs the float64 sum of single calls", grads, {k: g.cpu().numpy() for k, g in gsum.items()})
    _check_module("fp32 batch", logits, states, grads, xs, params, L, w)
    again = _run_module(m, bags, w)
    assert torch.equal(again[0], logits) and all(torch.equal(again[2][k], grads[k]) for k in grads)


@pytest.mark.parametrize("name", EC.names("ragged"))
def test_ragged_table_alone(name):
    case, inp, got = _replay(name)
    again = _run(case, inp)
    _same_bits(name + " second run", got, again, [k for k, v in got.items() if v is not None])


# ---- 4. 1 .. 16 queries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.names("queries"))
def test_query_counts(name):
    case, inp, got = _replay(name)
    assert tuple(got["Z"].shape) == (1, case.P, EC.width(case)) and tuple(got["dE"].shape) == (case.P, EC.width(case))


@pytest.mark.parametrize("P", [0, 17])
def test_query_counts_outside_the_kernels_raise(P):
    from vlsa_amd import VlsaNativeError
    from vlsa_amd import functional as VF
    bags, xp, _ = IH.source(17, "act", 960, DEV)
    with pytest.raises(VlsaNativeError):
        VF.ilra_pool_bags(bags, torch.zeros(P, 512, device=DEV), None)
    with pytest.raises(VlsaNativeError):
        VF.ilra_pool_bags(bags, torch.zeros(P, 256, device=DEV), xp)


# ---- 5. the caps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.names("cap"))
def test_both_sides_of_the_caps(name):
    _replay(name)


# ---- 6. peaks ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.names("rising"))
def test_maximum_that_rises_on_every_tile(name):
    _replay(name)


@pytest.mark.parametrize("name", EC.names("spike"))
def test_one_row_far_ahead(name):
    """the parts without the row merge with weight 0 (N = 700); Z of that query is the row, every gradient stays finite"""
    case, inp, got = _replay(name)
    IH.rel(f"{name} Z[query {EC.SPIKE_Q}] vs the row itself", got["Z"][0, EC.SPIKE_Q], inp["rows"][0][-1])
    assert all(bool(torch.isfinite(v).all()) for v in got.values() if v is not None)


# ---- 7. the chunk limit and short bags -------------------------------------------------------------------------------------------------
def test_64_bags_forward_and_backward():
    """one chunk of 64 bags of 1 .. 40 rows: [64, 256] b~ gradients, the column sums and dE over the parts of 64 bags"""
    L = 2
    params = IC.make_params(L, 4, 970)
    m = IH.build_model(L, 4, params, DEV)
    sizes = [1 + (7 * i) % 40 for i in range(64)]
    assert min(sizes) == 1 and max(sizes) == 40
    bags = [IH.bag(IC.make_bag(n, "bf16", 971 + i), "bf16", DEV) for i, n in enumerate(sizes)]
    w = np.random.RandomState(972).standard_normal((64, 4)).astype(np.float32)
    logits, states, grads = _run_module(m, bags, w)
    assert len(states) == 1 and tuple(states[0]["Z0"].shape) == (64, 8, 512)
    singles, gsum = [], None
    for i, x in enumerate(bags):
        out, _, g = _run_module(m, [x], w[i:i + 1])
        singles.append(out)
        gsum = {k: v.double() for k, v in g.items()} if gsum is None else {k: gsum[k] + g[k].double() for k in g}
    assert torch.equal(logits, torch.cat(singles)), float((logits - torch.cat(singles)).abs().max())
    IH.check_grads("64 bags vs the float64 sum of single calls", grads, {k: g.cpu().numpy() for k, g in gsum.items()})
    again = _run_module(m, bags, w)
    assert torch.equal(again[0], logits) and all(torch.equal(again[2][k], grads[k]) for k in grads)


@pytest.mark.parametrize("name", EC.names("chunk"))
def test_64_bags_alone(name):
    """the pooling and the row map at B = 64 directly against float64: per-bag Z and b~ gradients, dE over the parts of 64 bags, the
    folded bias gradients"""
    _replay(name)


@pytest.mark.parametrize("name", EC.names("short"))
def test_bags_shorter_than_the_column_segments(name):
    _replay(name)


# ---- every instantiation -------------------------------------------------------------------------------------------------------------
KERNELS = "k_ip_forward|k_ip_backward|k_ip_merge|k_ip_reduce|k_rm_forward|k_rm_backward|k_rm_wgrad|k_rm_reduce|k_rm_colsum|k_rm_colfold"


def _instantiation(key):
    """a profiler kernel name -> {(kernel, row type, D[, DX])}: demangled ``k_x<float, 512, false>``, or mangled where the demangler
    does not know the bf16 type (``k_xIDF16bLi512ELb0EE...``)"""
    mt = re.search(rf"({KERNELS})I(DF16b|f)Li(\d+)E(?:Lb([01])E)?E", key)
    if mt:
        dx = () if mt.group(4) is None else ("true" if mt.group(4) == "1" else "false",)
        return {(mt.group(1), "float" if mt.group(2) == "f" else "bf16", mt.group(3)) + dx}
    mt = re.search(rf"({KERNELS})(?:<([^>]*)>)?", key)
    if not mt:
        return set()
    args = [a.strip() for a in (mt.group(2) or "").split(",") if a.strip()]
    if args:
        args[0] = "float" if args[0] == "float" else "bf16"
    return {(mt.group(1),) + tuple(args)}


def _kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    found = set()
    for e in prof.key_averages():
        found |= _instantiation(e.key)
    return found


ROWS = {"bf16": ("bf16", "512"), "f32": ("float", "512"), "act": ("float", "256")}


def test_every_instantiation_is_launched_by_a_case_compared_with_float64():
    """the ragged tables (all three sources) and the no-gradient tables, each checked against float64 while the profiler lists the
    kernels: every instantiation of ilra.hip and its five plain kernels"""
    def go():
        for name in EC.names("ragged") + EC.names("nograd"):
            _replay(name)
    found = _kernels(go)
    print("[ilra instantiations]", sorted(found))
    want = {("k_ip_merge",), ("k_ip_reduce",), ("k_rm_reduce",), ("k_rm_colsum",), ("k_rm_colfold",)}
    for src, r in ROWS.items():
        want |= {("k_ip_forward",) + r, ("k_rm_forward",) + r, ("k_rm_wgrad",) + r, ("k_ip_backward",) + r + ("false",), ("k_rm_backward",) + r + ("false",)}
    want |= {("k_ip_backward", "float", "256", "true"), ("k_rm_backward", "float", "256", "true")}
    assert len(want) == 22 and want <= found, sorted(want - found)
