"""The case table of tests/clip_shape_cases.py against the host-side row plan of the CLIP towers (no GPU): every case sits where the
table says -- M, M_pad, max_len, the prefix the plan keeps, the keys per key workgroup, the backward's route -- so a later edit of the
table cannot silently move a case off the boundary it is there for; and the seeded inputs meet the condition the GPU gates rest on."""
import pytest
import torch

import clip_shape_cases as SC
import clip_text_cases as CC
from vlsa_amd.prompt_encoder import last_token_rows

ALL = SC.CASES + list(SC.EXTRA.values())


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_case_sits_where_the_table_says(case):
    pseudo = SC.pseudo_tokens(case.rows)
    assert pseudo.argmax(dim=-1).tolist() == [r - 1 for r in case.rows]            # the <eot> slot carries the row's maximum
    rp = last_token_rows(pseudo, SC.CTX, case.L)
    M_pad = (rp["M"] + 95) // 96 * 96                     # (_RowPlan: whole 16-, 32- and 48-row workgroup tiles)
    assert (rp["M"], M_pad, rp["max_len"], rp["prefix_len"]) == (case.M, case.M_pad, case.max_len, case.prefix_len)
    assert rp["n_seq"] == len(case.rows)
    rows = [b - a + rp["prefix_len"] for a, b in zip(rp["seq_row0"], rp["seq_row0"][1:])]
    assert rows == list(case.rows)
    assert rp["M"] == rp["prefix_len"] + sum(r - rp["prefix_len"] for r in case.rows)
    # every row a token row, the prompt's last one its <eot> position
    assert rp["row_src"] == rp["row_pos"] and all(rp["cls_keep"])
    assert [rp["row_pos"][b - 1] for b in rp["seq_row0"][1:]] == [r - 1 for r in case.rows]
    assert SC.keys_per_workgroup(case) == case.kpb
    c = CC.TOWERS[case.tower]
    assert c["heads"] * 64 == c["width"] == 768 and c["ctx"] == SC.CTX
    assert CC.WEIGHT_SCALES[SC.TOWER_SEEDS[case.tower]] == (3.5, 3.5)
    if case.route is not None:
        assert case.route == SC.route_of(case) == ("fused" if case.M <= 128 else "stage")
        assert case.max_len <= 64                                                   # the attention backward holds 64 rows


def test_table_covers_both_sides_of_every_threshold():
    main = [c for c in SC.CASES if c.tower == "w768x2"]
    assert {96, 97, 112, 113, 128, 129, 160, 161} <= {c.M for c in main if c.L == 0 and len(set(c.rows)) <= 2}
    assert {c.kpb for c in main if len(c.rows) == 12 and c.M < 128 and c.L > 0} == {0, 1, 2, 3, 4}
    g = SC.get
    # ragged prompts on either route, with an exact 64-row prompt in the backward; a single prompt; a two-row prompt with a gradient
    assert g("ragged100").rows == g("o768_ragged100").rows == (3, 16, 17, 64) and g("ragged100").route == "fused"
    assert g("ragged154").route == "stage" and len(set(g("ragged154").rows)) == 7 and g("ragged154").max_len == 64
    assert g("one").rows == (13,) and g("sot_eot").rows == (2, 13) and g("sot_eot").route == "fused"
    # forward only: both sides of the second key chunk, the last position, the shortest prompt, past 160 and 192 rows
    assert g("fwd_edges").rows == (64, 65, 66, 77, 2) and g("fwd_edges").route is None and g("fwd_edges").M_pad == 288
    # the prefix plan at the fused route's last row count and past it; 64 rows with a prefix; a ticket forced by K, not by L
    assert (g("L8M128").M, g("L8M128").kpb, g("L8M129").M, g("L8M129").kpb) == (128, 1, 129, 0)
    assert (g("S64pfx").max_len, g("S64pfx").prefix_len, g("S64pfx").kpb) == (64, 25, 2)
    assert (len(g("K16L17").rows), g("K16L17").kpb, g("L17").kpb) == (16, 0, 3)
    assert len(set(g("raggedpfx").rows)) > 3 and g("raggedpfx").prefix_len == 9
    assert g("fallback").L == 8 and g("fallback").prefix_len == 0 and min(g("fallback").rows) == g("fallback").L
    # the other towers
    assert CC.TOWERS[g("x3_L9").tower]["layers"] == 3 and g("x3_L9")[2:] == g("L9")[2:]
    assert CC.TOWERS[g("o768_ragged100").tower]["out_dim"] == 768 and g("o768_ragged100")[2:] == g("ragged100")[2:]
    assert set(SC.TRAIN_CASES) == {"ragged100", "L9", "L25", "ragged154"}
    # the HuggingFace-layout cases leave room to cut the rows short of 77 positions
    assert all(max(g(n).rows) + 3 < SC.CTX and CC.TOWERS[g(n).tower]["out_dim"] == 768 for n, _ in SC.HF_CASES)


def test_inputs_are_seeded_and_prefix_cases_share_their_prefix():
    case = SC.get("raggedpfx")
    a, b = SC.make_inputs(case), SC.make_inputs(case)
    assert all(torch.equal(a[k], b[k]) for k in ("prefix", "own", "pseudo", "G"))
    emb = SC.assemble(a["prefix"], a["own"])
    assert emb.shape == (6, 77, 768) and all(torch.equal(emb[s, :9], a["prefix"]) for s in range(6))
    assert 0.015 < float(emb.std()) < 0.025
    assert SC.make_inputs(SC.get("one"))["prefix"] is None


@pytest.mark.parametrize("name", SC.CONDITION_CASES)
def test_fp32_truth_stays_within_a_quarter_of_the_gate(name):
    """The yardstick of the GPU gates: the fp32 CPU truth's own distance from the float64 one on the same inputs, by the measures the GPU
    test applies (absolute on features, per prompt on d embedding, per tensor on d prefix).  The inputs are acceptable only while it stays
    <= 2.5e-5 -- a quarter of the 1e-4 gate; if this fails, change the seed or the scale, not the gate."""
    case = SC.get(name)
    e_feat, rel_own, rel_pfx, r64 = SC.yardstick(case)
    line = f"[clip shapes yardstick {name}] fp32 vs float64 truth: features {e_feat:.2e}; d own rows per prompt {rel_own:.2e}"
    if case.L > 0:
        line += f"; d prefix {rel_pfx:.2e}"
    print(line + f"; largest activation input {r64['stats']['act_input_absmax']:.2f}")
    assert r64["stats"]["act_input_absmax"] > 6.0                                   # QuickGELU in the sigmoid's tails
    # the slots behind <eot> get an exactly-zero gradient in the truth, the <eot> slot itself does not
    for s, r in enumerate(case.rows):
        assert not r64["d_emb"][s, r:].any()
        assert r64["d_emb"][s, r - 1].any()
    assert e_feat <= SC.YARDSTICK_MAX and rel_own <= SC.YARDSTICK_MAX and rel_pfx <= SC.YARDSTICK_MAX
