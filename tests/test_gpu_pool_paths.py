"""The single-bag pooling kernels of vlsa_amd/csrc/mil_pool.hip on every dispatch path -- scalar, vector, strided, misaligned, at the
512-partial cap -- against float64 references (tests/pool_path_cases.py), plus the short-row top-k, the batched scored pooling and
the query pooling.  Every test prints its figure before it asserts; the last test prints the worst figure per entry point and family.

Layouts the Python wrappers would copy (odd row strides, misaligned pointers) go through the raw C entry points with ctypes."""
import ctypes

import pytest
import torch

import pool_path_cases as PC

pytestmark = pytest.mark.gpu
WORST = {}            # (entry, family) -> (figure in units of its gate, case id)


def _dev():
    return torch.device("cuda", 0)


def _ids(cases):
    return [PC.case_id(c) for c in cases]


def _upload(case, inp):
    """the case's X on the GPU in the layout it asks for: (tensor that owns the memory, [N, D] view, pointer to the first element)"""
    entry, dtype, N, D, ldx, off, kind = case
    base, _ = PC.embed(inp["X"], ldx, off)
    dbase = base.to(_dev())
    view = PC.view_of(dbase, N, D, ldx, off)
    ptr = dbase.data_ptr() + off                 # (an empty view answers data_ptr() == 0)
    assert dbase.data_ptr() % 16 == 0 and (N == 0 or view.data_ptr() == ptr)
    return dbase, view, ctypes.c_void_p(ptr)


def _scores(a):
    """the scores on the GPU, one spare element behind them"""
    buf = torch.zeros(a.numel() + 1, dtype=torch.float32, device=_dev())
    buf[:-1] = a.to(_dev())
    return buf[:-1]


def _note(case, figure, gate, what=""):
    """print the figure, keep the worst per (entry, family)"""
    path = PC.case_path(case)
    key = (case[0], path[0])
    rel = figure / gate if gate else figure
    print(f"[pool paths] {PC.case_id(case)} {path} {what}: {figure:.3e} (gate {gate:.1e})")
    if key not in WORST or not rel <= WORST[key][0]:
        WORST[key] = (rel, PC.case_id(case))


def _big_rows_gate(case, gate, torch_err):
    """``big_rows`` only: max(gate, 4 x the error of torch's fp32 evaluation, both against float64) -- fp32 rounding of a 1e8 dynamic
    range is no kernel bug, and the kernel merges up to 512 partials where torch sums once.  One case needs it,
    rowdot-bf16-N257-D512-ld516-o0-big_rows (the 1e4-scaled row's dot cancels): k_rowdot 2.03e-5 of the largest dot against the 2e-5
    gate, torch's fp32 row dot 2.4e-5 to 6.5e-5 depending on the CPU's matmul (tests/test_pool_path_cases_cpu.py prints it).  Every
    other big_rows case measured at most 4.4e-6 (rowdot) and 3e-7 (scored pooling), inside the plain gates."""
    return max(gate, 4.0 * torch_err) if case[6] == "big_rows" else gate


def _pool_partials(lib, nat, F, ptr, case, a):
    entry, dtype, N, D, ldx, off, kind = case
    G = lib.vlsa_pool_num_partials(N)
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=_dev())  # noqa: E731
    pm, pl, pacc = f(G, nat.P_STRIDE), f(G, nat.P_STRIDE), f(G + 1, 1, D)       # (one spare row behind the partials)
    nat.check(lib.vlsa_scored_pool_partial(ptr, nat.DT_F32 if dtype == "f32" else nat.DT_BF16, N, ldx, D, F._p(a), F._p(pm), F._p(pl),
                                           F._p(pacc), F._stream()), "vlsa_scored_pool_partial")
    return F.vlfan_merge(pm, pl, pacc[:G])[2][0]


def _scored_pool(case, inp, with_scores=True):
    """pooled [D]: a contiguous aligned bag through the public wrapper, every other layout through the raw entry point + merge"""
    from vlsa_amd import _native as nat, functional as F
    entry, dtype, N, D, ldx, off, kind = case
    keep, view, ptr = _upload(case, inp)
    a = _scores(inp["a"]) if with_scores else None
    if ldx == D and off == 0:
        assert F._bag2d(view).data_ptr() == view.data_ptr()
        out = F.scored_pool(view, a)
    else:
        out = _pool_partials(nat.load(), nat, F, ptr, case, a)
    torch.cuda.synchronize()
    return out.double().cpu()


@pytest.mark.parametrize("case", PC.cases_of("scored_pool"), ids=_ids(PC.cases_of("scored_pool")))
def test_scored_pool(case):
    inp = PC.make_inputs(case)
    ref = PC.ref_scored_pool(inp["X"], inp["a"])
    scale = max(1.0, ref.abs().max().item())
    torch_err = (torch.softmax(inp["a"], dim=0) @ inp["X"].float() - ref).abs().max().item() / scale
    gate = _big_rows_gate(case, PC.GATE_POOL, torch_err)
    err = (_scored_pool(case, inp) - ref).abs().max().item() / scale
    _note(case, err, gate, "softmax")
    assert err <= gate
    if case[6] == "flat" or (case[6] == "randn" and case[2] in (5, 65, 32_773)):        # scores == NULL: the mean
        mref = PC.ref_scored_pool(inp["X"], None)
        merr = (_scored_pool(case, inp, with_scores=False) - mref).abs().max().item() / max(1.0, mref.abs().max().item())
        _note(case, merr, PC.GATE_POOL, "mean")
        assert merr <= PC.GATE_POOL


def _colmax(case, inp):
    from vlsa_amd import _native as nat, functional as F
    entry, dtype, N, D, ldx, off, kind = case
    lib = nat.load()
    keep, view, ptr = _upload(case, inp)
    G = lib.vlsa_pool_num_partials(N)
    part = torch.zeros(G + 1, D, dtype=torch.float32, device=_dev())
    out = torch.zeros(D, dtype=torch.float32, device=_dev())
    nat.check(lib.vlsa_colmax(ptr, nat.DT_F32 if dtype == "f32" else nat.DT_BF16, N, ldx, D, F._p(part), F._p(out), F._stream()), "vlsa_colmax")
    if ldx == D and off == 0:
        assert torch.equal(F.colmax(view).view(torch.int32), out.view(torch.int32))       # the public wrapper: the same launch
    torch.cuda.synchronize()
    return out.cpu()


def _bits_differ(got, ref, zero_col=None):
    """number of entries whose bits differ; the all-zero column of ``ties`` (fmaxf may return either zero) counts by value"""
    diff = got.view(torch.int32) != ref.view(torch.int32)
    if zero_col is not None:
        diff[zero_col] = got[zero_col] != ref[zero_col]
    return int(diff.sum())


@pytest.mark.parametrize("case", PC.cases_of("colmax"), ids=_ids(PC.cases_of("colmax")))
def test_colmax(case):
    """bit-equal to the float64 maximum (exact in fp32).  The all-zero column of ``ties`` holds zeros of both signs; fmaxf(-0.0, +0.0)
    may return either, so that one column is compared with == and every other column by its bits."""
    inp = PC.make_inputs(case)
    ref = PC.ref_colmax(inp["X"]).float()
    got = _colmax(case, inp)
    bad = _bits_differ(got, ref, case[3] - 1 if case[6] == "ties" else None)
    _note(case, float(bad), 0.0, "columns that differ")
    assert bad == 0


def _rowdot(case, inp):
    from vlsa_amd import _native as nat, functional as F
    entry, dtype, N, D, ldx, off, kind = case
    keep, view, ptr = _upload(case, inp)
    out = torch.zeros(N + 1, dtype=torch.float32, device=_dev())
    v = inp["v"].to(_dev())
    nat.check(nat.load().vlsa_rowdot(ptr, nat.DT_F32 if dtype == "f32" else nat.DT_BF16, N, ldx, D, F._p(v), F._p(out), F._stream()), "vlsa_rowdot")
    if ldx == D and off == 0:
        assert torch.equal(F.rowdot(view, v), out[:N])
    torch.cuda.synchronize()
    assert out[N].item() == 0.0
    return out[:N].double().cpu()


@pytest.mark.parametrize("case", PC.cases_of("rowdot"), ids=_ids(PC.cases_of("rowdot")))
def test_rowdot(case):
    inp = PC.make_inputs(case)
    ref = PC.ref_rowdot(inp["X"], inp["v"])
    scale = max(1.0, ref.abs().max().item())
    gate = _big_rows_gate(case, PC.GATE_ROWDOT, (inp["X"].float() @ inp["v"] - ref).abs().max().item() / scale)
    err = (_rowdot(case, inp) - ref).abs().max().item() / scale
    _note(case, err, gate)
    assert err <= gate


@pytest.mark.parametrize("case", PC.cases_of("pool_backward"), ids=_ids(PC.cases_of("pool_backward")))
def test_scored_pool_backward_entry_point(case):
    """vlsa_scored_pool_backward with the forward's statistics and pooled row taken from float64, so that only this kernel is measured;
    on the scalar conditions it answers VLSA_EUNSUPPORTED."""
    from vlsa_amd import _native as nat, functional as F
    entry, dtype, N, D, ldx, off, kind = case
    inp = PC.make_inputs(case)
    keep, view, ptr = _upload(case, inp)
    a, v = _scores(inp["a"]), inp["v"].to(_dev())
    m2v, lv = PC.stats_log2(inp["a"])
    m2 = torch.full((nat.P_STRIDE,), m2v, dtype=torch.float32, device=_dev())
    l = torch.full((nat.P_STRIDE,), lv, dtype=torch.float32, device=_dev())
    pooled = PC.ref_scored_pool(inp["X"], inp["a"]).float().to(_dev())
    da = torch.zeros(N + 1, dtype=torch.float32, device=_dev())
    rc = nat.load().vlsa_scored_pool_backward(ptr, nat.DT_F32 if dtype == "f32" else nat.DT_BF16, N, ldx, D, F._p(a), F._p(m2), F._p(l),
                                              F._p(pooled), F._p(v), F._p(da), F._stream())
    torch.cuda.synchronize()
    if PC.case_path(case) == "unsupported":
        assert rc == nat.EUNSUPPORTED and da.abs().max().item() == 0.0
        return
    assert rc == nat.OK and da[N].item() == 0.0
    err = (da[:N].double().cpu() - PC.ref_scored_pool_backward(inp["X"], inp["a"], inp["v"])).abs().max().item()
    scale = PC.backward_scale(inp["X"], inp["a"], inp["v"])
    err = err / scale if scale > 0 else err
    _note(case, err, PC.GATE_BACKWARD)
    assert err <= PC.GATE_BACKWARD


@pytest.mark.parametrize("case", PC.cases_of("normalize"), ids=_ids(PC.cases_of("normalize")))
def test_normalize_many(case):
    from vlsa_amd import _native as nat, functional as F
    entry, dtype, N, D, ldx, off, kind = case
    inp = PC.make_inputs(case)
    keep, view, ptr = _upload(case, inp)
    obuf = torch.zeros(N * D + 8, dtype=torch.float32, device=_dev())
    ooff = 1 if kind == "misaligned_out" else 0
    rc = nat.load().vlsa_normalize_many(ptr, nat.DT_F32 if dtype == "f32" else nat.DT_BF16, N, ldx, D, ctypes.c_void_p(obuf.data_ptr() + 4 * ooff),
                                        F._stream())
    torch.cuda.synchronize()
    path = PC.case_path(case)
    if not isinstance(path, tuple):
        assert rc == (nat.EUNSUPPORTED if path == "unsupported" else nat.EINVAL) and obuf.abs().max().item() == 0.0
        return
    assert rc == nat.OK and obuf[N * D:].abs().max().item() == 0.0
    if N == 0:
        return
    err = (obuf[:N * D].view(N, D).double().cpu() - PC.ref_normalize(inp["X"])).abs().max().item()
    _note(case, err, PC.GATE_NORMALIZE)
    assert err <= PC.GATE_NORMALIZE
    if ldx == D or ldx == 640:
        assert torch.equal(F.normalize_many(view), obuf[:N * D].view(N, D))           # the public wrapper keeps such a view


# ---- the two paths on the same bag ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("N", [6, 65, 257])
@pytest.mark.parametrize("kind", ("randn",) + PC.POOL_KINDS + ("ties",))
def test_scalar_and_vector_paths_agree(kind, N, dtype):
    """one logical [N, 512] bag, contiguous (vector kernels) and behind a row stride of 513 / 516 elements (scalar kernels): scored
    pooling within twice the gate, colmax bit-equal"""
    vec = ("scored_pool", dtype, N, 512, 512, 0, kind)
    inp = PC.make_inputs(vec)
    sca = vec[:4] + (PC.ODD_STRIDE[dtype], 0, kind)
    assert PC.case_path(vec) == ("vec", 2 if dtype == "f32" else 1) and PC.case_path(sca) == ("scalar", 8)
    pv, ps = _scored_pool(vec, inp), _scored_pool(sca, inp)
    ref = PC.ref_scored_pool(inp["X"], inp["a"])
    err = (pv - ps).abs().max().item() / max(1.0, ref.abs().max().item())
    cv, cs = _colmax(("colmax",) + vec[1:], inp), _colmax(("colmax",) + sca[1:], inp)
    bad = _bits_differ(cv, cs)
    print(f"[pool paths] paths agree {dtype} N{N} {kind}: pooled differ by {err:.3e} (gate {2 * PC.GATE_POOL:.0e}), colmax bits differ in {bad}")
    assert err <= 2 * PC.GATE_POOL
    assert bad == 0


# ---- backward through the Python wrapper: the fused kernel and the rowdot + torch branch ---------------------------------------------
@pytest.mark.parametrize("dtype,D", [("f32", 512), ("bf16", 512), ("f32", 513), ("bf16", 516)])
@pytest.mark.parametrize("N", [1, 65, 257])
@pytest.mark.parametrize("kind", ["randn", "one_hot"])
def test_scored_pool_backward_both_python_branches(kind, N, dtype, D):
    from vlsa_amd import functional as F
    case = ("pool_backward", dtype, N, D, D, 0, kind)
    inp = PC.make_inputs(case)
    Xd = inp["X"].to(_dev())
    a = inp["a"].to(_dev()).requires_grad_(True)
    F.scored_pool(Xd, a).backward(inp["v"].to(_dev()))
    torch.cuda.synchronize()
    a64 = inp["a"].double().requires_grad_(True)
    (torch.softmax(a64, dim=0) @ inp["X"].double()).backward(inp["v"].double())
    assert (a64.grad - PC.ref_scored_pool_backward(inp["X"], inp["a"], inp["v"])).abs().max().item() <= 1e-12 * max(1.0, a64.grad.abs().max().item())
    scale = PC.backward_scale(inp["X"], inp["a"], inp["v"])
    err = (a.grad.double().cpu() - a64.grad).abs().max().item()
    err = err / scale if scale > 0 else err
    fused = D % (8 if dtype == "bf16" else 4) == 0
    print(f"[pool paths] backward {'fused' if fused else 'rowdot + torch'} {dtype} N{N} D{D} {kind}: {err:.3e} (gate {PC.GATE_BACKWARD:.0e})")
    key = ("python_backward", "fused" if fused else "rowdot")
    if key not in WORST or not err / PC.GATE_BACKWARD <= WORST[key][0]:
        WORST[key] = (err / PC.GATE_BACKWARD, f"{dtype}-N{N}-D{D}-{kind}")
    assert err <= PC.GATE_BACKWARD


# ---- single-stage top-k at short rows -------------------------------------------------------------------------------------------------
def _topk_rows(N, k, g):
    """rows as in test_topk_mean_two_stage (ties, all negative, winners at either end), one whose k-th and (k + 1)-th values are equal
    and one with -inf among the losers (where there are losers)"""
    S = torch.randn(7, N, generator=g)
    S[1, : N // 3] = 0.25
    S[2] = -S[2].abs()
    S[3, -7:] = 10.0
    S[4, :3] = torch.tensor([9.0, 8.0, 7.0])[:min(3, N)]
    S[5, : min(k + 1, N)] = 5.0
    if k < N:
        losers = S[6].argsort()[: max(1, (N - k) // 2)]
        S[6, losers] = float("-inf")
    return S


@pytest.mark.parametrize("N", [1, 2, 31, 32, 33, 255, 256, 257, 4095, 4096])
def test_topk_mean_single_stage(N):
    from vlsa_amd import _native as nat, functional as F
    lib = nat.load()
    for k in sorted({1, 2, 31, 32, N, N + 1}):
        if 32 < k < N:
            continue
        S = _topk_rows(N, k, torch.Generator().manual_seed(7000 + 37 * N + k))
        ref = PC.ref_topk_mean(S, k)
        gate = PC.GATE_TOPK * max(1.0, ref.abs().max().item())
        Sd = S.to(_dev())
        got = F.topk_mean(Sd, k).double().cpu()
        raw = torch.zeros(S.shape[0], dtype=torch.float32, device=_dev())
        nat.check(lib.vlsa_topk_mean(F._p(Sd), S.shape[0], N, k, 1.0, F._p(raw), F._stream()), "vlsa_topk_mean")
        e1, e2 = (got - ref).abs().max().item(), (raw.double().cpu() - ref).abs().max().item()
        print(f"[pool paths] topk_mean N{N} k{k}: F.topk_mean {e1:.3e}, vlsa_topk_mean {e2:.3e} (gate {gate:.1e})")
        key = ("topk_mean", "single")
        if key not in WORST or not max(e1, e2) / gate <= WORST[key][0]:
            WORST[key] = (max(e1, e2) / gate, f"N{N}-k{k}")
        assert e1 <= gate and e2 <= gate


@pytest.mark.parametrize("N,k", [(5, 8), (4097, 8), (4097, 32)])
def test_topk_values_are_selected_not_summed(N, k):
    from vlsa_amd import _native as nat, functional as F
    lib = nat.load()
    S = _topk_rows(N, k, torch.Generator().manual_seed(7100 + N + k))
    Sd = S.to(_dev())
    ws = torch.zeros(max(4, lib.vlsa_topk_workspace_bytes(S.shape[0], N, k)), dtype=torch.uint8, device=_dev())
    vals = torch.zeros(S.shape[0], k, dtype=torch.float32, device=_dev())
    nat.check(lib.vlsa_topk_values(F._p(Sd), S.shape[0], N, k, F._p(ws), F._p(vals), F._stream()), "vlsa_topk_values")
    ref = torch.full((S.shape[0], k), float("-inf"))
    ref[:, : min(k, N)] = S.topk(min(k, N), dim=1).values
    assert torch.equal(vals.cpu().view(torch.int32), ref.view(torch.int32))


# ---- batched scored pooling over a descriptor table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("with_scores", [True, False])
@pytest.mark.parametrize("sizes,strided", [(list(range(1, 65)), None), ([5, 130, 63], 1), ([63], None)])
def test_pool_rows_batched(sizes, strided, with_scores, dtype):
    """B = 64 bags of 1 .. 64 rows: most of a bag's 8 partials own no row; B = 3 with one bag behind ldx = 640; B = 1 (64 partials) at
    N = 63.  Against float64 per bag, and against the single-bag scored_pool to twice the gate."""
    from vlsa_amd import _native as nat, functional as F
    from vlsa_amd.bag_tables import _stage_table, bag_rows
    g = torch.Generator().manual_seed(7200 + len(sizes))
    host = [torch.randn(n, 512, generator=g).to(PC.TORCH_DT[dtype]) for n in sizes]
    keep, bags = [], []
    for i, x in enumerate(host):
        base, _ = PC.embed(x, 640 if i == strided else 512, 0)
        keep.append(base.to(_dev()))
        bags.append(PC.view_of(keep[-1], x.shape[0], 512, 640 if i == strided else 512, 0))
    a_host = [torch.randn(n, generator=g) * 3 for n in sizes]
    a = torch.cat(a_host).to(_dev()) if with_scores else None
    offs = torch.tensor([0] + sizes[:-1]).cumsum(0).to(torch.int64)
    a_off = offs.to(_dev()) if with_scores else None
    desc = _stage_table(bag_rows(bags), _dev(), "test_pool_rows_batched")
    pooled, _, _ = F.pool_rows(desc, len(sizes), nat.DT_F32 if dtype == "f32" else nat.DT_BF16, a, a_off)
    torch.cuda.synchronize()
    worst = worst_single = 0.0
    for i, x in enumerate(host):
        ai = a_host[i] if with_scores else None
        ref = PC.ref_scored_pool(x, ai)
        scale = max(1.0, ref.abs().max().item())
        worst = max(worst, (pooled[i].double().cpu() - ref).abs().max().item() / scale)
        single = F.scored_pool(bags[i], None if ai is None else ai.to(_dev()))
        worst_single = max(worst_single, (pooled[i] - single).abs().max().item() / scale)
    print(f"[pool paths] pool_rows B{len(sizes)} {dtype} scores={with_scores}: vs float64 {worst:.3e} (gate {PC.GATE_POOL:.0e}), "
          f"vs single-bag {worst_single:.3e} (gate {2 * PC.GATE_POOL:.0e})")
    key = ("pool_rows", "vec")
    if key not in WORST or not worst / PC.GATE_POOL <= WORST[key][0]:
        WORST[key] = (worst / PC.GATE_POOL, f"B{len(sizes)}-{dtype}-scores{with_scores}")
    assert worst <= PC.GATE_POOL and worst_single <= 2 * PC.GATE_POOL


# ---- query pooling over the P aggregated rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hid", [1, 3, 5, 64, 257])
@pytest.mark.parametrize("P", [1, 2, 16])
@pytest.mark.parametrize("D", [8, 512, 1024])
def test_query_pool_attention(D, P, hid):
    """(Gated_)Attention_Pooling over [B, P, D] rows, B in {1, 5}, gated and not, raw scores and softmax weights, against
    raw = w2 . (tanh(Wa x + ba) [* sigmoid(Wg x + bg)]) + c;  attn = softmax_P(raw);  pooled = attn @ rows   in float64"""
    from vlsa_amd import _native as nat, functional as F
    lib = nat.load()
    g = torch.Generator().manual_seed(7300 + 100 * hid + 10 * P + D)
    u = lambda *s, b: (torch.rand(*s, generator=g) * 2 - 1) * b  # noqa: E731
    worst = 0.0
    for B in (1, 5):
        rows = torch.randn(B, P, D, generator=g)
        Wa, ba, Wg, bg = u(hid, D, b=3.0 / D ** 0.5), u(hid, b=0.05), u(hid, D, b=3.0 / D ** 0.5), u(hid, b=0.05)
        w2, c = u(hid, b=1.0 / hid ** 0.5), u(1, b=0.06)
        dv = lambda t: t.to(_dev())  # noqa: E731
        d_rows, d_Wa, d_ba, d_Wg, d_bg, d_w2, d_c = map(dv, (rows, Wa, ba, Wg, bg, w2, c))
        for gated in (False, True):
            e = torch.tanh(rows.double() @ Wa.double().T + ba.double())
            if gated:
                e = e * torch.sigmoid(rows.double() @ Wg.double().T + bg.double())
            raw = e @ w2.double() + c.double()                                   # [B, P]
            attn = torch.softmax(raw, dim=1)
            ref_pooled = torch.einsum("bp,bpd->bd", attn, rows.double())
            for want_raw in (0, 1):
                ws = torch.zeros(B * ((hid + 3) // 4) * nat.P_STRIDE, dtype=torch.float32, device=_dev())
                pooled = torch.zeros(B, D, dtype=torch.float32, device=_dev())
                scores = torch.zeros(B, P, dtype=torch.float32, device=_dev())
                nat.check(lib.vlsa_query_pool_attention(F._p(d_rows), B, P, D, F._p(d_Wa), F._p(d_ba), F._p(d_Wg) if gated else None,
                                                        F._p(d_bg) if gated else None, F._p(d_w2), F._p(d_c), hid, want_raw, F._p(ws),
                                                        F._p(pooled), F._p(scores), F._stream()), "vlsa_query_pool_attention")
                torch.cuda.synchronize()
                ep = (pooled.double().cpu() - ref_pooled).abs().max().item()
                es = (scores.double().cpu() - (raw if want_raw else attn)).abs().max().item()
                print(f"[pool paths] query pool hid{hid} P{P} D{D} B{B} gated={gated} raw={want_raw}: pooled {ep:.3e}, scores {es:.3e} "
                      f"(gate {PC.GATE_QPOOL:.0e})")
                worst = max(worst, ep, es)
                assert ep <= PC.GATE_QPOOL and es <= PC.GATE_QPOOL
    key = ("query_pool", "any")
    if key not in WORST or not worst / PC.GATE_QPOOL <= WORST[key][0]:
        WORST[key] = (worst / PC.GATE_QPOOL, f"hid{hid}-P{P}-D{D}")


def test_num_partials_at_the_cap_and_worst_figures(capsys):
    """(runs last) the partial count on the GPU machine's library, and the worst figure of this file per entry point and family"""
    from vlsa_amd import _native as nat
    lib = nat.load()
    for N in PC.ROWS_CAP:
        assert lib.vlsa_pool_num_partials(N) == min(512, -(-N // 64))
    with capsys.disabled():
        print()
        for (entry, fam), (rel, cid) in sorted(WORST.items()):
            print(f"[pool paths] worst {entry:16s} {fam:7s}: {rel:.3f} of its gate at {cid}")
