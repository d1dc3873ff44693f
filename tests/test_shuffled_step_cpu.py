"""Host side of the reshuffled training step (TrainStep.set_epoch / step_next, functional.BagSlots, vlsa_batch_gather): what is declared,
bound and refused without a GPU."""
import ctypes
from ctypes import c_int, c_int64, c_void_p

import numpy as np
import pytest
import torch

from abi_helpers import declared_symbols


def test_header_declares_the_gather_and_the_binding_types_it():
    from vlsa_amd import _native
    assert "vlsa_batch_gather" in declared_symbols() and "vlsa_batch_gather" in _native.exported_symbols()
    V = c_void_p
    # (src_desc, t_all, e_all, M, order, L, B, cursor, slot_desc, t_slot, e_slot, status, stream), typed by hand from the declaration
    assert _native._SIGNATURES["vlsa_batch_gather"] == (c_int, [V, V, V, c_int64, V, c_int64, c_int, V, V, V, V, V, V])
    assert hasattr(_native.load(), "vlsa_batch_gather")
    assert (_native.GATHER_BAD_CURSOR, _native.GATHER_BAD_INDEX) == (1, 2)
    assert _native.ABI_VERSION == 1 and "vlsa_bag_desc" in _native.STRUCTS


def test_gather_refuses_bad_arguments_before_any_launch():
    """the argument check returns before the launch: no GPU is touched"""
    from vlsa_amd import _native
    lib = _native.load()
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.cast(buf, c_void_p)
    assert lib.vlsa_batch_gather(p, p, p, 4, p, 4, lib.vlsa_batch_max_bags() + 1, p, p, p, p, p, None) == _native.EINVAL
    assert lib.vlsa_batch_gather(p, p, p, 4, p, 4, 0, p, p, p, p, p, None) == _native.EINVAL
    assert lib.vlsa_batch_gather(p, p, p, 0, p, 4, 2, p, p, p, p, p, None) == _native.EINVAL
    assert lib.vlsa_batch_gather(p, p, p, 4, p, -1, 2, p, p, p, p, p, None) == _native.EINVAL
    for hole in range(12):
        if hole in (3, 5, 6):
            continue                                          # (M, L, B: by value)
        args = [p, p, p, 4, p, 4, 2, p, p, p, p, p]
        args[hole] = None
        assert lib.vlsa_batch_gather(*args, None) == _native.EINVAL, hole


def _host_set(M):
    """a BagSet over host tensors through its internal constructor (the public one refuses CPU tensors): enough for the host-side checks"""
    from vlsa_amd.functional import BagSet
    bags = [torch.zeros(3 + i, 512) for i in range(M)]
    rows = np.asarray([(x.data_ptr(), x.shape[0], 512) for x in bags], dtype=np.int64)
    return BagSet(bags, _rows=rows)


def _stepper():
    from vlsa_amd.train_step import TrainStep
    w = torch.nn.Parameter(torch.zeros(4))
    return TrainStep(torch.nn.Identity(), lambda *a: None, torch.optim.SGD([w], lr=0.1))


@pytest.mark.parametrize("order", [[0, 1, 5], [0, -1, 2], [0.0, 1.0, 2.0], [True, False], [], [[0, 1], [2, 3]], np.array([0, 1, 7]),
                                   torch.tensor([0, 1, 2.5]), torch.tensor([4, 5])])
def test_set_epoch_refuses_an_order_that_is_not_integers_inside_the_source(order):
    ts = _stepper()
    t_all, e_all = torch.zeros(5, dtype=torch.int64), torch.zeros(5)
    with pytest.raises(ValueError):
        ts.set_epoch(_host_set(5), t_all, e_all, order, 2)


def test_set_epoch_refuses_a_source_that_is_no_bagset_and_a_batch_above_the_source():
    ts = _stepper()
    t_all, e_all = torch.zeros(5, dtype=torch.int64), torch.zeros(5)
    with pytest.raises(ValueError):
        ts.set_epoch([torch.zeros(3, 512)] * 5, t_all, e_all, [0, 1, 2], 2)
    with pytest.raises(ValueError):
        ts.set_epoch(_host_set(5), t_all, e_all, [0, 1, 2], 6)
    with pytest.raises(RuntimeError):
        ts.step_next()                                        # no epoch was begun


def test_follow_drops_everything_derived_from_the_previous_rows():
    """sub-sets, groups and the chunk plans ``_ChunkPlan.of`` keeps on a BagSet (row offsets, tile tables, buffer sizes): a plan of the
    previous batch against the refilled table would be an out-of-bounds write"""
    from vlsa_amd.functional import BagSlots, _ChunkPlan
    src = _host_set(6)
    s = BagSlots(src, 2)
    assert s.sizes == (3, 4) and s.chunk(0, 2) is s

    class Plan(_ChunkPlan):
        def __init__(self, bags):
            self.sizes = bags.sizes

    first = Plan.of(s)
    assert Plan.of(s) is first and first.sizes == (3, 4)          # kept while the rows stay
    sub = s.chunk(1, 1)
    s._groups[0] = 5
    s.follow([5, 2])
    assert s.sizes == (8, 5) and s[0] is src[5] and s[1] is src[2] and (s.rows == src.rows[[5, 2]]).all()
    assert Plan.of(s) is not first and Plan.of(s).sizes == (8, 5)
    assert s.chunk(1, 1) is not sub and s.chunk(1, 1).sizes == (5,) and not s._groups
    with pytest.raises(ValueError):
        s.follow([1])


def test_bagslots_refuses_more_bags_than_a_batched_launch_takes():
    from vlsa_amd import _native
    from vlsa_amd.functional import BagSlots
    cap = _native.load().vlsa_batch_max_bags()
    assert cap == 64
    with pytest.raises(ValueError, match="64"):
        BagSlots(_host_set(cap + 6), cap + 1)
    with pytest.raises(ValueError):
        BagSlots(_host_set(4), 0)
    with pytest.raises(ValueError):
        BagSlots([torch.zeros(3, 512)] * 4, 2)
    with pytest.raises(ValueError):
        BagSlots(_host_set(4), 2, t_all=torch.zeros(3, dtype=torch.int64))
