"""CPU-side checks of the batched MaxMIL / MeanMIL entry points (vlsa_colmax_batch, vlsa_pool_dx_batch, vlsa_gather_rows_batch and
their host-side queries): exported, declared in the header and bound, they refuse bad arguments on the host -- before anything is
launched, so no GPU is needed -- and a bag's part count is a function of its row count alone."""
import ctypes
import re

import pytest

from abi_helpers import HEADER_TEXT

NEW = ("vlsa_colmax_part_rows", "vlsa_colmax_parts", "vlsa_colmax_workspace_bytes", "vlsa_colmax_batch", "vlsa_pool_dx_tile_rows",
       "vlsa_pool_dx_batch", "vlsa_gather_rows_batch")


@pytest.fixture(scope="module")
def lib():
    from vlsa_amd import build, _native
    build.build_native()
    return _native.load()


def test_new_symbols_exported_declared_and_bound(lib):
    from vlsa_amd import _native
    for name in NEW:
        assert hasattr(lib, name)
        assert re.search(r"\b" + name + r"\s*\(", HEADER_TEXT), f"{name} not declared in include/vlsa_hip.h"
        assert name in _native.exported_symbols()
    assert lib.vlsa_abi_version() == 1


# any non-null address: every call below must be refused before it dereferences or launches anything
P = ctypes.c_void_p(0x1000)


def _colmax(lib, B=2, D=512, dt=1, desc=P, ps=P, n_parts=4, ws=P, out=P, idx=P):
    return lib.vlsa_colmax_batch(desc, B, dt, D, ps, n_parts, ws, out, idx, None)


def _dx(lib, B=2, mode=1, dxd=P, desc=P, idx=P, dp=P, ts=P, n_tiles=4):
    return lib.vlsa_pool_dx_batch(dxd, desc, B, mode, idx, dp, ts, n_tiles, None)


def _gather(lib, B=2, dt=1, desc=P, idx=P, out=P):
    return lib.vlsa_gather_rows_batch(desc, B, dt, idx, out, None)


@pytest.mark.parametrize("call", [_colmax, _dx, _gather])
def test_bad_batch_sizes_and_null_tables_are_refused(lib, call):
    bad = {lib.vlsa_error_string(-1)}
    for kw in ({"B": 0}, {"B": 65}, {"B": -3}, {"desc": None}, {"idx": None}):
        rc = call(lib, **kw)
        assert rc < 0 and lib.vlsa_error_string(rc) in bad, (call.__name__, kw, rc)


def test_widths_dtypes_nulls_short_tables_and_modes_are_refused(lib):
    for kw in ({"D": 256}, {"D": 1024}, {"dt": 7}, {"ps": None}, {"ws": None}, {"out": None}, {"n_parts": 1}, {"n_parts": 0},
               {"B": 3, "n_parts": 2}):
        assert _colmax(lib, **kw) < 0, kw
    for kw in ({"mode": 2}, {"mode": -1}, {"dxd": None}, {"dp": None}, {"ts": None}, {"n_tiles": 1}, {"B": 5, "n_tiles": 4}):
        assert _dx(lib, **kw) < 0, kw
    for kw in ({"dt": 7}, {"out": None}):
        assert _gather(lib, **kw) < 0, kw


def test_part_count_is_a_function_of_the_row_count_alone(lib):
    rows = lib.vlsa_colmax_part_rows()
    assert rows >= 1 and lib.vlsa_pool_dx_tile_rows() >= 1
    sizes = [1, 2, rows - 1, rows, rows + 1, 2 * rows + 3, 2798, 50000, 10 ** 6, 10 ** 9, 1 << 40]
    parts = [lib.vlsa_colmax_parts(n) for n in sizes]
    assert all(p >= 1 for p in parts)
    assert parts == sorted(parts)                                          # non-decreasing in N
    assert parts == [lib.vlsa_colmax_parts(n) for n in sizes]              # equal for equal N
    assert lib.vlsa_colmax_parts(rows) == 1 and lib.vlsa_colmax_parts(rows + 1) == 2
    assert all(p <= n for p, n in zip(parts, sizes))                       # every part owns at least one row
    for n_parts in (1, 4, 64 * 512):
        assert lib.vlsa_colmax_workspace_bytes(n_parts) >= n_parts * 512 * 8
