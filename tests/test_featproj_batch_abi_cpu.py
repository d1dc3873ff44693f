"""CPU-side checks of the batched Feat_Projecter entry points (vlsa_feat_project_batch, vlsa_feat_project_batch_tile_rows,
vlsa_feat_project_rowstats_batch): exported, declared in the header and bound, and they refuse bad arguments on the host with the
stated codes -- before anything is launched, so no GPU is needed."""
import ctypes
import re

import pytest

from abi_helpers import HEADER_TEXT

NEW = ("vlsa_feat_project_batch", "vlsa_feat_project_batch_tile_rows", "vlsa_feat_project_rowstats_batch")
EINVAL, EUNSUPPORTED = -1, -2          # include/vlsa_hip.h
BF16, F32 = 1, 0


@pytest.fixture(scope="module")
def lib():
    from vlsa_amd import build, _native
    build.build_native()
    return _native.load()


def test_new_symbols_exported_declared_and_bound(lib):
    from vlsa_amd import _native
    assert (_native.DT_BF16, _native.DT_F32) == (BF16, F32)
    for name in NEW:
        assert hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", HEADER_TEXT), f"{name} not declared in include/vlsa_hip.h"
        assert name in _native.exported_symbols()
    assert lib.vlsa_abi_version() == 1


# any non-null address: every call below must be refused before it dereferences or launches anything
P = ctypes.c_void_p(0x1000)


def _fwd(lib, desc=P, B=2, dt=BF16, D=512, prep=P, ts=P, n_tiles=4, tile_rows=32, Y=P, off=P, stats=P):
    return lib.vlsa_feat_project_batch(desc, B, dt, D, prep, 1e-5, ts, n_tiles, tile_rows, Y, off, stats, None)


def _rowstats(lib, dy=P, B=2, y=P, off=P, total=100, prep=P, stats=P):
    return lib.vlsa_feat_project_rowstats_batch(dy, B, y, off, total, prep, stats, None)


def test_forward_refuses_nulls_batch_sizes_and_tile_counts_as_invalid(lib):
    for kw in ({"desc": None}, {"prep": None}, {"ts": None}, {"Y": None}, {"off": None}, {"B": 0}, {"B": 65}, {"B": -3}, {"n_tiles": 0},
               {"n_tiles": -1}, {"tile_rows": 16}, {"tile_rows": 48}, {"tile_rows": 256}, {"tile_rows": 128, "dt": F32}):
        assert _fwd(lib, **kw) == EINVAL, kw
    # stats = NULL is the inference form: refused here only for another reason
    assert _fwd(lib, stats=None, B=0) == EINVAL


def test_forward_refuses_other_widths_and_dtypes_as_unsupported(lib):
    for kw in ({"D": 256}, {"D": 1024}, {"D": 0}, {"dt": 2}, {"dt": 7}, {"dt": -1}):
        assert _fwd(lib, **kw) == EUNSUPPORTED, kw


def test_rowstats_refuses_nulls_and_sizes(lib):
    for kw in ({"dy": None}, {"y": None}, {"off": None}, {"prep": None}, {"stats": None}, {"B": 0}, {"B": 65}, {"total": 0}):
        assert _rowstats(lib, **kw) == EINVAL, kw


def test_tile_height_follows_the_single_bag_thresholds_on_the_total(lib):
    """feat_project_impl: bf16 128 rows from 120 x 128 rows on, 64 from 120 x 64, else 32; fp32 64 from 120 x 64, else 32"""
    f = lib.vlsa_feat_project_batch_tile_rows
    assert [f(BF16, n) for n in (1, 7679, 7680, 15359, 15360, 1_600_000)] == [32, 32, 64, 64, 128, 128]
    assert [f(F32, n) for n in (1, 7679, 7680, 15360, 1_600_000)] == [32, 32, 64, 64, 64]
    assert f(7, 1000) == 0
