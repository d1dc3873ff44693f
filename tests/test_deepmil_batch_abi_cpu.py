"""CPU-side checks of the batched DeepMIL training entry points (vlsa_gated_scores_batch_train, vlsa_attn_pool_backward_batch,
vlsa_attn_scores_backward_dx_seeded): exported, declared in the header and bound, and they refuse bad arguments on the host --
before anything is launched, so no GPU is needed."""
import ctypes
import re

import pytest

from abi_helpers import HEADER_TEXT

NEW = ("vlsa_gated_scores_batch_train", "vlsa_attn_pool_backward_batch", "vlsa_attn_scores_backward_dx_seeded")


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


def _scores(lib, B=2, D=512, desc=P, prep=P, ts=P, a=P, off=P, drop=0.25, seed=P, dt=1):
    return lib.vlsa_gated_scores_batch_train(desc, B, dt, D, prep, 1, ts, 4, 64, a, off, 100, drop, seed, None)


def _bwd(lib, B=2, D=512, desc=P, ts=P, a=P, m2=P, l=P, pooled=P, dp=P, ws=P, seed=P, drop=0.25, dt=1):
    return lib.vlsa_attn_pool_backward_batch(desc, B, dt, D, P, 1, ts, 4, a, P, m2, l, 16, pooled, dp, ws, P, P, None, None, drop,
                                             seed, None)


def _dx(lib, B=2, D=512, desc=P, dxd=P, da=P, seed=P, drop=0.25):
    return lib.vlsa_attn_scores_backward_dx_seeded(desc, dxd, B, 1, D, P, P, 1, P, 4, da, P, P, P, drop, seed, None)


@pytest.mark.parametrize("call", [_scores, _bwd, _dx])
def test_bad_batch_sizes_width_and_nulls_are_refused(lib, call):
    from vlsa_amd import _native
    bad = {_native.load().vlsa_error_string(-1)}
    for kw in ({"B": 0}, {"B": 65}, {"B": -3}, {"desc": None}, {"seed": None}):
        rc = call(lib, **kw)
        assert rc < 0 and lib.vlsa_error_string(rc) in bad, (call.__name__, kw, rc)
    rc = call(lib, D=256)
    assert rc < 0, (call.__name__, "D=256", rc)
    rc = call(lib, D=1024)
    assert rc < 0, (call.__name__, "D=1024", rc)


def test_other_nulls_and_rates_are_refused(lib):
    for kw in ({"prep": None}, {"ts": None}, {"a": None}, {"off": None}, {"drop": 1.0}, {"drop": -0.1}, {"dt": 7}):
        assert _scores(lib, **kw) < 0, kw
    for kw in ({"ts": None}, {"a": None}, {"m2": None}, {"l": None}, {"pooled": None}, {"dp": None}, {"ws": None}, {"drop": 1.0},
               {"dt": 7}):
        assert _bwd(lib, **kw) < 0, kw
    for kw in ({"dxd": None}, {"da": None}, {"drop": 1.0}):
        assert _dx(lib, **kw) < 0, kw
