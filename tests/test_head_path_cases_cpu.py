"""The case list of tests/head_path_cases.py without a GPU: every reachable dispatch path of the head and tail kernels has its cases
at the edges that flip it, the recipes do what they say, and torch's own fp32 evaluation of every case meets -- against the float64
reference -- the gate the GPU test applies: the gates are reachable by a correct fp32 kernel."""
from collections import Counter

import torch

import head_path_cases as HC


def test_every_reachable_path_has_cases(capsys):
    table = Counter((c.entry, HC.case_path(c)) for c in HC.CASES)
    with capsys.disabled():
        print()
        for (entry, path), n in sorted(table.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))):
            print(f"[head paths] {entry:17s} {' / '.join(path):45s}: {n:3d} cases")
    req = HC.required_paths()
    for row in req:
        assert table[row] > 0, row
    assert set(table) <= set(req), sorted(set(table) - set(req))          # no case runs a path the table does not name
    assert all(isinstance(HC.case_path(c), tuple) for c in HC.CASES)
    ids = [c.id for c in HC.CASES]
    assert len(set(ids)) == len(ids), [i for i, n in Counter(ids).items() if n > 1]
    assert set(c.entry for c in HC.CASES) == set(HC.ENTRIES)


def test_the_edges_the_dispatch_flips_at():
    by = lambda e: HC.cases_of(e)  # noqa: E731
    # widths: every one on the entries that take them; 512 only on the fused tail and the MFMA adapter
    for e in ("head_forward", "head_batch", "head_backward"):
        assert {c.D for c in by(e)} >= set(HC.WIDTHS), e
    assert {c.D for c in by("head_batch_text")} >= set(HC.WIDTHS) and {c.B for c in by("head_batch_text")} >= set(HC.BAGS)
    assert {c.D for c in by("merge_head_batch")} >= set(HC.WIDTHS)
    assert {c.D for c in by("merge_head")} >= {8, 256, 512, 768, 1024}
    assert all(c.D == 512 for c in HC.CASES if HC.case_path(c)[0] == "fused" or "mfma" in HC.case_path(c))
    # bags
    assert {c.B for c in by("head_batch")} >= set(HC.BAGS) and {c.B for c in by("head_backward")} >= set(HC.BAGS)
    mfma = {c.B for c in by("head_batch") if "mfma" in HC.case_path(c)}
    assert mfma >= {16, 17, 31, 32, 33, 63, 64, 65, 129}
    valu = [(c.B, c.D) for c in by("head_batch") if "valu" in HC.case_path(c)]
    assert any(B >= 16 and D != 512 for B, D in valu) and any(B % 8 and D != 512 for B, D in valu) and any(B < 16 and D == 512 for B, D in valu)
    # the `pre` predicate: K 16 / 17 below, at and above 512 columns
    fin = {(c.D, c.K): HC.case_path(c)[-1] for c in by("head_batch") if HC.case_path(c)[0] == "rows"}
    assert fin[(252, 16)] == fin[(512, 16)] == "pre" and fin[(252, 17)] == fin[(512, 17)] == fin[(516, 16)] == fin[(516, 17)] == "inplace"
    # the ticketed head: half-empty last workgroup, one workgroup, the batched grid with and without the adapter
    assert HC.head_nb(508, True) == 64 and HC.head_nb(512, True) == 64 and HC.head_nb(516, True) == 65 and HC.head_nb(1024, False) == 1
    assert any(c.D % 8 == 4 and c.adapter for c in by("head_forward"))
    grid = [c for c in by("head_batch") if HC.case_path(c)[-1] == "grid_b"]
    assert {c.layout for c in grid} == {"contig", "inplace"} and {c.adapter for c in grid} == {True, False}
    assert {c.mode for c in grid if c.layout == "inplace"} == {"given", "mean", "max", "weight"} and {c.mode for c in grid if c.layout == "contig"} == {"given"}
    # merges
    assert {(c.mode, HC.case_path(c)[0]) for c in by("merge_head")} >= {("given", "unfused"), ("max", "unfused"), ("mean", "fused"), ("weight", "fused")}
    assert {c.G for c in by("merge_head") if HC.case_path(c)[0] == "fused"} >= set(HC.G_SINGLE)
    assert {c.G for c in by("merge_head") if HC.case_path(c)[0] == "unfused"} >= set(HC.G_SINGLE)
    for lay in ("contig", "strided"):
        assert {c.G for c in by("merge_head_batch") if c.layout == lay} >= set(HC.G_BATCH)
    sw = {(c.G, c.P, c.mode) for c in by("merge_head_batch")}
    assert sw >= {(G, P, m) for G in (8, 9) for P in (1, 16) for m in ("max", "weight")}
    assert HC.expected_path("merge_head_batch", B=3, G=8, P=2)[0] == "small" and HC.expected_path("merge_head_batch", B=3, G=9, P=2)[0] == "batch"
    for e in ("merge_head", "merge_head_batch"):
        assert {c.recipe for c in by(e)} >= set(HC.MERGE_RECIPES)
    # the backward: the dW / db carry (an adapter with more than 64 bags), both NULL-able gradients both ways
    assert sum(1 for c in by("head_backward") if c.adapter and c.B > 64) >= 6
    assert {(c.gv, c.gt) for c in by("head_backward")} == {(a, b) for a in (False, True) for b in (False, True)}
    assert HC.backward_counts(129, 516, True) == (3, 17 * 17, 9, 65) and HC.backward_counts(64, 512, False) == (0, 16 * 8, 4, 64)
    assert {c.D for c in by("head_backward")} >= {2, 33}
    # the query chain
    assert {(c.nq, c.gated) for c in by("query_chain")} == {(1, False), (2, False), (13, False), (17, False), (2, True), (13, True), (17, True)}
    # pooling modes, incidence, bias
    for e in ("head_forward", "head_batch", "head_batch_text", "merge_head", "merge_head_batch"):
        assert {c.mode for c in by(e)} >= set(HC.MODES) and {c.inc for c in by(e)} == {True, False}, e
    assert any(not c.bias and c.adapter for c in by("head_forward")) and any(c.ls == 0.0 for c in by("head_forward"))
    assert any(c.ls == HC.LS_100 for c in by("head_batch"))
    # refusals
    for entry, what, kw in HC.REFUSALS:
        assert HC.refusal_path(entry, kw) == "einval", (entry, what)


def test_recipes_do_what_they_say():
    seen = Counter()
    for c in HC.CASES:
        if c.recipe == "randn" or c.entry == "query_chain":
            continue
        inp = HC.make_inputs(c)
        ref = HC.reference(c, inp)
        seen[c.recipe] += 1
        for name, t in ref.items():
            assert torch.isfinite(t).all(), (c.id, name)
        if c.recipe == "parallel" and "logits" in ref:
            s = float(inp["ls"].double().exp())
            assert ref["logits"][0, 0].item() > s * (1 - 1e-5), c.id
            assert c.K == 1 or ref["logits"][0, 1].item() < -s * (1 - 1e-5), c.id
        elif c.recipe in ("norm1e3", "norm1e-6"):
            t = (inp.get("rows") if "rows" in inp else inp["pacc"]).abs().max().item()
            assert (t > 1e2) if c.recipe == "norm1e3" else (t < 1e-4), c.id
            n = inp["T"].norm(dim=-1)
            assert (n.min() > 1e3) if c.recipe == "norm1e3" else (n.max() < 1e-3)
        elif c.recipe == "zero_pooled":
            assert not c.adapter and inp["rows"][0].abs().max().item() == 0
            if "vhat" in ref:
                assert ref["vhat"][0].abs().max().item() == 0 and ref["logits"][0].abs().max().item() == 0
            if "drows" in ref and inp["dlogits"].abs().max() > 0:
                assert ref["drows"][0].abs().max().item() > 1e9              # g / 1e-12: the clamp's gradient
        elif c.recipe == "max_ties":
            assert c.mode == "max" and torch.equal(inp["rows"][:, 0, 0::2], inp["rows"][:, 1, 0::2])
        elif c.recipe == "sat_weight":
            assert torch.softmax(inp["pw"].double(), 0).max().item() > 1 - 1e-15
        elif c.recipe == "dl_onehot":
            assert (inp["dlogits"] != 0).sum().item() == 1
        elif c.recipe == "dl_zero":
            assert all(t.abs().max().item() == 0 for t in ref.values())
        elif c.recipe.startswith("empty_"):
            gi = {"empty_first": 0, "empty_middle": c.G // 2, "empty_last": c.G - 1}[c.recipe]
            assert (inp["pm"][:, gi] == float("-inf")).all() and inp["pl"][:, gi].abs().max() == 0 and inp["pacc"][:, gi].abs().max() == 0
            if c.G > 1:                                                        # the record weighs nothing: the merge without it
                keep = [g for g in range(c.G) if g != gi]
                m2, l, out = HC.merge64(inp["pm"][:, keep], inp["pl"][:, keep], inp["pacc"][:, keep], c.P)
                assert torch.allclose(out, ref["out"], rtol=1e-12, atol=0) and torch.allclose(l, ref["l"], rtol=1e-12, atol=0)
        elif c.recipe == "spread60":
            assert inp["pm"].max().item() > 40 and inp["pm"].min().item() < -40 and inp["pm"].abs().max().item() <= 60
    assert set(seen) >= set(HC.FWD_RECIPES) | set(HC.MERGE_RECIPES) | set(HC.BWD_RECIPES) | {"ls100"}


def test_strided_layout_has_spare_floats_and_keeps_the_abi():
    c = next(c for c in HC.cases_of("merge_head_batch") if c.layout == "strided")
    sm, sl, sa, bm, bl, ba, om, ol, oo = HC.strided_layout(c)
    assert sm > 16 and sl > 16 and sa > c.P * c.D and bm > c.G * sm and bl > c.G * sl and ba > c.G * sa and oo > c.P * c.D
    assert sa % 4 == 0 and ba % 4 == 0 and oo % 4 == 0
    c2 = next(c for c in HC.cases_of("merge_head_batch") if c.layout == "contig")
    assert HC.strided_layout(c2) == [16, 16, c2.P * c2.D, 16 * c2.G, 16 * c2.G, c2.G * c2.P * c2.D, 16, 16, c2.P * c2.D]


def test_fp32_torch_meets_every_gate_against_float64(capsys):
    """For every case and output: error of torch's fp32 CPU evaluation against the float64 reference, in units of the gate the GPU test
    applies.  Every gate must leave 2x room (ratio <= 0.5): no recipe needs a wider gate than the suite's own."""
    worst = {}
    for c in HC.CASES:
        inp = HC.make_inputs(c)
        ref, got = HC.reference(c, inp), HC.fp32_eval(c, inp)
        assert set(ref) == set(got)
        for label, e, g in HC.judged(c, got, ref):
            r = HC.ratio(e, g)
            key = (c.entry, c.recipe)
            if r >= worst.get(key, (-1.0,))[0]:
                worst[key] = (r, label, c.id)
            assert r <= 0.5, (c.id, label, e, g)
    with capsys.disabled():
        print()
        for (entry, recipe), (r, label, cid) in sorted(worst.items()):
            print(f"[head paths] fp32 torch vs float64, worst {entry:17s} {recipe:12s}: {r:.3f} of its gate ({label}) at {cid}")
    assert {k[0] for k in worst} == set(HC.ENTRIES)


def test_parts_and_scaled_gates():
    c = next(c for c in HC.cases_of("head_backward") if c.recipe == "zero_pooled")
    inp = HC.make_inputs(c)
    ref = HC.reference(c, inp)
    rows = {label: g for label, e, g in HC.judged(c, ref, ref)}
    assert rows["drows [bag 0]"] > 1e6 * rows["drows [bags 1..]"] > 0
    c = next(c for c in HC.cases_of("head_forward") if c.recipe == "norm1e-6")
    ref = HC.reference(c, HC.make_inputs(c))
    assert HC.gate(c, "pooled", ref["pooled"]) < 1e-9 and HC.gate(c, "logits", ref["logits"]) == HC.GATE_LOGITS
