"""The case table of tests/text_shape_cases.py against the host-side row plan (no GPU): every case sits where the table says -- M, M_pad,
max_len, the prefix the plan keeps, the keys per key workgroup -- so a later edit of the table cannot silently move a case off the
boundary it is there for; and the seeded inputs meet the condition the GPU gates rest on."""
import pytest
import torch

import text_cases as TC
import text_shape_cases as SC
from vlsa_amd.prompt_encoder import compact_rows

ALL = SC.CASES + list(SC.EXTRA.values())


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_case_sits_where_the_table_says(case):
    rp = compact_rows(SC.pseudo_tokens(case.lens), SC.CTX, case.L)
    M_pad = (rp["M"] + 95) // 96 * 96                     # (_RowPlan: whole 16-, 32- and 48-row workgroup tiles)
    assert (rp["M"], M_pad, rp["max_len"], rp["prefix_len"]) == (case.M, case.M_pad, case.max_len, case.prefix_len)
    assert rp["n_seq"] == len(case.lens)
    # rows per prompt: n + 2 (a sentence without any pad: 127 positions + the CLS row, which then attends to itself)
    rows = [b - a + rp["prefix_len"] for a, b in zip(rp["seq_row0"], rp["seq_row0"][1:])]
    assert rows == [min(n + 2, SC.CTX) for n in case.lens]
    assert SC.keys_per_workgroup(case) == case.kpb
    d, heads = TC.TOWERS[case.tower]["width"], TC.TOWERS[case.tower]["heads"]
    assert heads * 64 == d
    if case.route is not None and d == 768 and case.name not in SC.EXTRA:
        assert case.route == ("fused" if case.M <= 128 else "stage")


def test_table_covers_both_sides_of_every_threshold():
    Ms = {c.M for c in SC.CASES if c.tower == "w768x2" and c.L == 0}
    assert {96, 97, 112, 113, 128, 129, 160, 161} <= Ms
    assert {c.kpb for c in SC.CASES if c.tower == "w768x2" and len(c.lens) == 12 and c.M <= 128 and c.L > 0} == {0, 1, 2, 3, 4}
    assert {SC.get(n).max_len for n in ("ragged100", "S64pfx")} == {64} and SC.get("S65").max_len == 65
    assert SC.get("fwd_edges").max_len == 128 and SC.get("fallback").prefix_len == 0
    assert SC.get("small_M1024").M == 1024 and SC.get("small_M1040").M > 1024
    # a CLS row that sees itself: only the sentence without a pad
    rp = compact_rows(SC.pseudo_tokens(SC.get("fwd_edges").lens), SC.CTX, 0)
    cls_rows = [r - 1 for r in rp["seq_row0"][1:]]
    assert [rp["cls_keep"][r] for r in cls_rows] == [0, 0, 0, 1, 0]


def test_inputs_are_seeded_and_prefix_cases_share_their_prefix():
    case = SC.get("raggedpfx")
    a, b = SC.make_inputs(case), SC.make_inputs(case)
    assert all(torch.equal(a[k], b[k]) for k in ("prefix", "own", "pseudo", "G"))
    emb = SC.assemble(a["prefix"], a["own"])
    assert emb.shape == (6, 127, 768) and all(torch.equal(emb[s, :9], a["prefix"]) for s in range(6))
    assert 0.015 < float(emb.std()) < 0.025
    assert SC.make_inputs(SC.get("one"))["prefix"] is None


@pytest.mark.parametrize("name", SC.CONDITION_CASES)
def test_fp32_oracle_stays_within_a_quarter_of_the_gate(name):
    """The yardstick of the GPU gates: the fp32 CPU oracle's own distance from the float64 one on the same inputs, by the measures the GPU
    test applies (absolute on features, per prompt on d embedding).  The inputs are acceptable only while it stays <= 2.5e-5 -- a quarter
    of the 1e-4 gate; if this fails, change the seed or the scale, not the gate."""
    case = SC.get(name)
    e_feat, rel_own, rel_pfx, r64 = SC.yardstick(case)
    line = f"[text shapes yardstick {name}] fp32 vs float64 oracle: features {e_feat:.2e}; d own rows per prompt {rel_own:.2e}"
    if case.L > 0:
        line += f"; d prefix {rel_pfx:.2e}"
    print(line)
    # the slots behind the first pad get an exactly-zero gradient in the reference
    for s, n in enumerate(case.lens):
        assert not r64["d_emb"][s, n + 1:].any()
        assert r64["d_emb"][s, n].any()                    # ... and the first pad slot does not: the CLS row sees it
    assert e_feat <= SC.YARDSTICK_MAX and rel_own <= SC.YARDSTICK_MAX and rel_pfx <= SC.YARDSTICK_MAX
