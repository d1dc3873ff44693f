"""The bags of tests/maxpool_cases.py really contain what their names say, and torch's CPU ``max`` -- the reference of the GPU tests --
names the FIRST maximal row of a column, ties between -0.0 and +0.0 included."""
import pytest
import torch

import maxpool_cases as MC


@pytest.fixture(scope="module")
def P():
    from vlsa_amd import build, _native
    build.build_native()
    return int(_native.load().vlsa_colmax_part_rows())


DTYPES = [torch.bfloat16, torch.float32]


def _first_max_by_hand(x):
    xf = x.float()
    v = xf.max(dim=0).values
    hit = xf == v[None, :]                        # (-0.0 == +0.0)
    rows = torch.arange(x.shape[0])[:, None].expand_as(hit)
    return torch.where(hit, rows, torch.full_like(rows, x.shape[0])).min(dim=0).values.to(torch.int32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_reference_names_the_first_maximal_row(P, dtype):
    for name, (x, (v, i)) in MC.build(P, dtype).items():
        assert x.dtype == dtype and x.shape[1] == 512 and v.shape == i.shape == (512,), name
        assert i.dtype == torch.int32 and int(i.min()) >= 0 and int(i.max()) < x.shape[0], name
        assert torch.equal(i, _first_max_by_hand(x)), name
        assert torch.equal(v, x.float()[i.long(), torch.arange(512)]), name
        assert not torch.isnan(x.float()).any(), name


@pytest.mark.parametrize("dtype", DTYPES)
def test_sizes_and_strides(P, dtype):
    c = MC.build(P, dtype)
    assert [c[k][0].shape[0] for k in MC.SIZES] == [1, 2, P - 1, P, P + 1, 2 * P + 3]
    assert c["slide_2798"][0].shape[0] == 2798
    x = c["strided"][0]
    assert x.stride() == (640, 1) and not x.is_contiguous() and (x.stride(0) * x.element_size()) % 16 == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_placed_maxima_and_ties(P, dtype):
    c = MC.build(P, dtype)
    x, (v, i) = c["max_in_first_row"]
    assert torch.equal(i, torch.zeros(512, dtype=torch.int32)) and (x.float()[1:] < 50).all()
    x, (v, i) = c["max_in_last_row"]
    assert torch.equal(i, torch.full((512,), x.shape[0] - 1, dtype=torch.int32)) and (x.float()[:-1] < 50).all()
    x, (v, i) = c["duplicate_across_parts"]
    assert x.shape[0] == 2 * P                                            # two parts: rows [0, P) and [P, 2 P)
    assert torch.equal(x[P - 1], x[P]) and (v == 40).all() and (x.float() == 40).sum(dim=0).min() >= 2
    assert ((x.float() == 40).sum(dim=0)[1::2] == 3).all()
    assert torch.equal(i, torch.full((512,), P - 1, dtype=torch.int32))   # the last row of part 0 wins


@pytest.mark.parametrize("dtype", DTYPES)
def test_special_columns(P, dtype):
    x, (v, i) = MC.build(P, dtype)["special_columns"]
    xf = x.float()
    assert (xf[:, 3] == 1.5).all() and i[3] == 0
    assert (xf[:, 5] < -2.9e38).all() and torch.isfinite(xf[:, 5]).all() and (xf[:, 5] == xf[0, 5]).all() and i[5] == 0
    assert torch.isinf(xf[:, 6]).all() and (xf[:, 6] < 0).all() and i[6] == 0 and v[6] == float("-inf")
    for col, first_negative in ((7, True), (8, False)):
        assert torch.signbit(xf[2, col]).item() == first_negative and torch.signbit(xf[4, col]).item() != first_negative
        assert xf[2, col] == 0 and xf[4, col] == 0 and (xf[:, col] <= 0).all()
        assert i[col] == 2 and v[col] == 0


def test_bf16_slide_has_tied_maxima(P):
    """seeded randn rounded to bf16 repeats its maximum within a column of 2 798 rows: the case where ``amax`` and ``max`` differ"""
    x, (v, i) = MC.build(P, torch.bfloat16)["slide_2798"]
    tied = ((x.float() == v[None, :]).sum(dim=0) > 1).sum().item()
    assert tied >= 5, tied
    x, (v, i) = MC.build(P, torch.float32)["slide_2798"]
    assert ((x == v[None, :]).sum(dim=0) > 1).sum().item() == 0
