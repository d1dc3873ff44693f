"""The case list of tests/pool_path_cases.py without a GPU: every reachable instantiation of the pooling kernels has its cases, the
recipes do what they say, the float64 references and torch's fp32 evaluation agree within the gates the GPU tests apply, and the
library's partial count follows its formula at the 512-partial cap."""
from collections import Counter

import pytest
import torch

import pool_path_cases as PC

OK_PATHS = [c for c in PC.CASES if isinstance(PC.case_path(c), tuple)]


def _table():
    return Counter((c[0], c[1]) + PC.case_path(c) for c in OK_PATHS)


def _required():
    """(entry, dtype, family, instantiation) rows that must not be empty"""
    rows = []
    for entry in ("scored_pool", "colmax"):
        rows += [(entry, dt, "scalar", dpl) for dt in ("f32", "bf16") for dpl in (4, 8, 12, 16)]
        rows += [(entry, "f32", "vec", nc) for nc in (1, 2, 3, 4)] + [(entry, "bf16", "vec", nc) for nc in (1, 2)]
    for entry in ("rowdot", "pool_backward", "normalize"):
        rows += [(entry, "f32", "vec", nc) for nc in (1, 2, 3, 4)] + [(entry, "bf16", "vec", nc) for nc in (1, 2)]
    rows += [("rowdot", dt, "scalar", 0) for dt in ("f32", "bf16")]
    return rows


def test_every_reachable_instantiation_has_cases(capsys):
    table = _table()
    with capsys.disabled():
        print()
        for row in sorted(table):
            print(f"[pool paths] {row[0]:14s} {row[1]:5s} {row[2]:7s} {row[3]:2d}: {table[row]:4d} cases")
    for row in _required():
        assert table[row] > 0, row
        rows_n = {c[2] for c in OK_PATHS if (c[0], c[1]) + PC.case_path(c) == row}
        assert {1, 5, 65} <= rows_n, (row, sorted(rows_n))
    assert not [c for c in PC.CASES if c[1] == "bf16" and isinstance(PC.case_path(c), tuple) and PC.case_path(c)[0] == "vec"
                and PC.case_path(c)[1] > 2], "bf16 NC 3 / 4 cannot be reached: D <= 1024"
    assert len(set(PC.CASES)) == len(PC.CASES)


def test_the_widths_strides_and_pointers_the_issue_names():
    have = {(c[0], c[1], c[3], c[4], c[5]) for c in PC.CASES}
    for entry in ("scored_pool", "colmax"):
        for dt in ("f32", "bf16"):
            for D in PC.SCALAR_WIDTHS[dt] + PC.VECTOR_WIDTHS[dt]:
                assert (entry, dt, D, D, 0) in have
            assert (entry, dt, 512, PC.ODD_STRIDE[dt], 0) in have and PC.expected_path(entry, dt, 512, PC.ODD_STRIDE[dt], 0) == ("scalar", 8)
            assert (entry, dt, 512, 512, PC.ESZ[dt]) in have and PC.expected_path(entry, dt, 512, 512, PC.ESZ[dt]) == ("scalar", 8)
            for ldx in (640, 1024):
                assert (entry, dt, 512, ldx, 0) in have and PC.expected_path(entry, dt, 512, ldx, 0)[0] == "vec"
    assert PC.expected_path("scored_pool", "f32", 513, 513, 0) == ("scalar", 12)
    assert PC.expected_path("colmax", "bf16", 1020, 1020, 0) == ("scalar", 16)
    assert PC.expected_path("scored_pool", "f32", 772, 772, 0) == ("vec", 4)
    assert PC.expected_path("rowdot", "f32", 1028, 1028, 0) == ("scalar", 0) and ("rowdot", "f32", 1028, 1028, 0) in have
    assert PC.expected_path("pool_backward", "f32", 513, 513, 0) == "unsupported"
    refusals = Counter(PC.case_path(c) for c in PC.CASES if not isinstance(PC.case_path(c), tuple))
    assert refusals["einval"] == 2 and refusals["unsupported"] >= 2 * (4 + 3)
    norm = {(c[1], c[3], c[4], c[5], c[6]): PC.case_path(c) for c in PC.cases_of("normalize")}
    assert norm[("f32", 6, 6, 0, "randn")] == norm[("bf16", 12, 12, 0, "randn")] == "unsupported"
    assert norm[("f32", 512, 513, 0, "randn")] == norm[("f32", 512, 512, 8, "randn")] == norm[("f32", 512, 512, 0, "misaligned_out")] == "unsupported"
    assert norm[("f32", 1028, 1028, 0, "randn")] == "einval"
    assert any(c[2] == 0 for c in PC.cases_of("normalize")) and any(c[6] == "tiny_rows" and c[4] != c[3] for c in PC.cases_of("normalize"))


def test_every_kind_runs_on_a_scalar_and_a_vector_kernel_and_the_cap_is_there():
    fam = {}
    for c in OK_PATHS:
        fam.setdefault(c[6], set()).add(PC.case_path(c)[0])
    for kind in ("randn",) + PC.POOL_KINDS + ("ties",):
        assert fam[kind] == {"scalar", "vec"}, (kind, fam[kind])
    for entry in ("scored_pool", "colmax", "rowdot"):
        for dt in ("f32", "bf16"):
            for ldx in (512, PC.ODD_STRIDE[dt]):
                assert {c[2] for c in PC.cases_of(entry) if c[1] == dt and c[4] == ldx and c[3] == 512} >= set(PC.ROWS_CAP)
    assert all(c[3] == 512 for c in PC.CASES if c[2] >= PC.ROWS_CAP[0])
    assert max(c[2] * c[4] * PC.ESZ[c[1]] for c in PC.CASES) < 70e6                         # bytes a case moves


def test_recipes_do_what_they_say():
    for c in PC.CASES:
        entry, dt, N, D, ldx, off, kind = c
        if kind == "randn" or N > 300:
            continue
        inp = PC.make_inputs(c)
        X, a = inp["X"].double(), inp["a"]
        w = PC.softmax64(a)
        if kind == "one_hot":
            assert w.max().item() >= 1 - 1e-12 and int(w.argmax()) == N // 2
            assert torch.equal(PC.ref_scored_pool(inp["X"], a).float(), inp["X"][N // 2].float())
        elif kind == "neg_inf_rows":
            assert torch.isfinite(PC.ref_scored_pool(inp["X"], a)).all() and torch.isfinite(PC.ref_scored_pool_backward(inp["X"], a, inp["v"])).all()
            assert w[:4].abs().max().item() == 0 and w[N - 1].item() == 0 and w.sum().item() == pytest.approx(1.0)
        elif kind in ("spike_last", "spike_first"):
            r = N - 1 if kind == "spike_last" else 0
            assert (X.argmax(dim=0) == r).all() and int(a.argmax()) == r
        elif kind == "flat":
            assert (PC.ref_scored_pool(inp["X"], a) - X.mean(dim=0)).abs().max().item() < 1e-12
        elif kind == "big_rows":
            assert X[N // 3].abs().max().item() > 1e3 and X[(2 * N) // 3].abs().max().item() < 1e-3
        elif kind == "ties":
            assert (X[:, 0] == X[:, 0].max()).sum().item() == 2 and (X[:, D - 1] == 0).all()
            assert torch.signbit(inp["X"][:, D - 1]).any() and not torch.signbit(inp["X"][:, D - 1]).all()


def test_embed_places_the_view_and_the_sentinel():
    X = PC.make_inputs(("colmax", "bf16", 5, 512, 516, 2, "randn"))["X"]
    base, view = PC.embed(X, 516, 2)
    assert torch.equal(view, X) and view.stride() == (516, 1) and (view.data_ptr() - base.data_ptr()) == 2
    assert torch.equal(PC.view_of(base, 5, 512, 516, 2), X)
    assert base.numel() == 6 * 516 + 1 and (base == PC.SENTINEL).sum().item() == base.numel() - 5 * 512


def _fp32_figure(c):
    """(error of torch's fp32 CPU evaluation against the float64 reference, the gate of the GPU test) -- both in the gate's own unit"""
    entry, dt, N, D, ldx, off, kind = c
    inp = PC.make_inputs(c)
    X, a, v = inp["X"], inp["a"], inp["v"]
    Xf = X.float()
    if entry == "scored_pool":
        ref = PC.ref_scored_pool(X, a)
        return (torch.softmax(a, dim=0) @ Xf - ref).abs().max().item() / max(1.0, ref.abs().max().item()), PC.GATE_POOL
    if entry == "colmax":
        return (Xf.max(dim=0).values.double() - PC.ref_colmax(X)).abs().max().item(), 0.0
    if entry == "rowdot":
        ref = PC.ref_rowdot(X, v)
        return (Xf @ v - ref).abs().max().item() / max(1.0, ref.abs().max().item()), PC.GATE_ROWDOT
    if entry == "pool_backward":
        A = torch.softmax(a, dim=0)
        got = A * (Xf @ v - (A @ Xf) @ v)
        return (got - PC.ref_scored_pool_backward(X, a, v)).abs().max().item() / PC.backward_scale(X, a, v), PC.GATE_BACKWARD
    ref = PC.ref_normalize(X)
    return (torch.nn.functional.normalize(Xf, dim=-1) - ref).abs().max().item(), PC.GATE_NORMALIZE


def test_references_agree_with_fp32_torch_within_the_gpu_gates(capsys):
    """the gates are not tighter than rounding alone allows: torch's own fp32 evaluation of every case (the N >= 32 704 ones at one
    N per entry point) meets them against the float64 references.  ``big_rows`` is the exception the GPU tests know about: a row
    dot of a 1e4-scaled row that happens to cancel leaves fp32 torch at 2.4e-5 of the largest dot, above the 2e-5 gate
    (rowdot-bf16-N257-D512-ld516-o0-big_rows); that kind is gated at max(gate, 4 x torch's fp32 error) there and only reported here."""
    worst, worst_big = {}, (0.0, "")
    for c in OK_PATHS:
        if c[2] == 0 or (c[2] >= PC.ROWS_CAP[0] and not (c[2] == 32_773 and c[4] == 512 and c[1] == "f32")):
            continue
        fig, gate = _fp32_figure(c)
        if c[6] == "big_rows":
            worst_big = max(worst_big, (fig / gate if gate else fig, PC.case_id(c)))
            continue
        if fig >= worst.get(c[0], (-1.0,))[0]:
            worst[c[0]] = (fig, gate, PC.case_id(c))
        assert fig <= gate, (PC.case_id(c), fig, gate)
    with capsys.disabled():
        print()
        for entry, (fig, gate, cid) in sorted(worst.items()):
            print(f"[pool paths] fp32 torch vs float64, worst {entry:14s}: {fig:.2e} (gate {gate:.0e}) at {cid}")
        print(f"[pool paths] fp32 torch vs float64, big_rows: at most {worst_big[0]:.2f} of its gate, at {worst_big[1]}")
    assert set(worst) == set(PC.ENTRIES)


def test_topk_reference():
    S = torch.tensor([[1.0, 5.0, 3.0, 5.0], [-1.0, -2.0, -3.0, float("-inf")]])
    assert PC.ref_topk_mean(S, 2).tolist() == [5.0, -1.5] and PC.ref_topk_mean(S, 9)[0].item() == 3.5


def test_num_partials_at_the_cap():
    from vlsa_amd import _native as nat
    lib = nat.load()
    for N in (1, 63, 64, 65, 127, 129, 257) + PC.ROWS_CAP + (10 ** 6,):
        assert lib.vlsa_pool_num_partials(N) == min(512, -(-N // 64)), N
    assert lib.vlsa_pool_num_partials(32_704) == 511 and lib.vlsa_pool_num_partials(32_705) == 512
