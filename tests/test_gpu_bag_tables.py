"""vlsa_amd.bag_tables on the device: the three ways a chunk's tables come about -- packed on the host into one upload, derived from
an uploaded descriptor by in-stream ops, written by vlsa_fill_one_bag_tables for a single bag -- hold the same words (the host layout
itself is checked word by word in test_bag_tables_cpu.py), DSMIL's part table equals its host restatement, and ``pool_rows`` is
bit-equal to the three launches it replaced."""
import ctypes

import numpy as np
import pytest
import torch

from test_bag_tables_cpu import BASE, HEIGHTS, SIZES, FakeBag, _chunks

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _fake(sizes):
    """bags nobody reads: addresses, sizes and strides for the tables alone"""
    bags = [FakeBag(BASE + (i << 24), n, 512 + 8 * (i % 3)) for i, n in enumerate(sizes)]
    for x in bags:
        x.device = DEV
    return bags


def test_device_tables_equal_host_tables():
    from vlsa_amd import _native as nat
    from vlsa_amd import bag_tables as BT
    from vlsa_amd import functional as VF
    lib = nat.load()
    for sizes in _chunks():
        bags = _fake(sizes)
        rows = BT.bag_rows(bags)
        dev = BT.ChunkTables.from_device(BT._stage_table(rows, DEV, "test"), tuple(sizes), nat.DT_BF16)
        for h in HEIGHTS:
            host = BT.ChunkTables.from_host(rows, nat.DT_BF16, h, DEV, "test")
            (a, na), (b, nb) = dev.tile_start(h), host.tile_start(h)
            assert a.is_cuda and b.is_cuda and a.dtype == b.dtype == torch.int32
            assert torch.equal(a.cpu(), b.cpu()) and na == nb == int(a[-1]), (sizes, h)
            assert torch.equal(dev.row_off.cpu(), host.row_off.cpu()) and torch.equal(dev.desc.cpu(), host.desc.cpu())
            assert host.p_tile_start(h) == (b.data_ptr(), nb) and dev.p_tile_start(h) == (a.data_ptr(), na)
        plan = VF.DsmilBagsPlan(bags)                                           # (a plain list: its descriptor is staged)
        parts = [int(lib.vlsa_dsmil_parts(n)) for n in sizes]
        assert plan.part_start.cpu().tolist() == [0] + np.cumsum(parts).tolist() and plan.n_parts == sum(parts)
        assert torch.equal(plan.a_off.cpu(), dev.row_off.cpu())


@pytest.mark.parametrize("two", [False, True], ids=["one_table", "two_tables"])
def test_one_bag_tables_written_on_the_device_equal_the_upload(two):
    from vlsa_amd import bag_tables as BT
    for n in SIZES:
        x = torch.empty(n, 512, dtype=torch.bfloat16, device=DEV)
        g = torch.empty(n, 512, dtype=torch.float32, device=DEV) if two else None
        for h in HEIGHTS:
            one = BT.ChunkTables.from_one_bag(x, h, g)
            host = BT.ChunkTables.from_host(BT.bag_rows([x]), BT._dt(x), h, DEV, "test", BT.bag_rows([g]) if two else None)
            words = 8 if two else 5                                              # (the one-bag buffer is 8 words whatever it holds)
            assert torch.equal(one.keep.cpu()[:words], host.keep.cpu()), (n, h)
            assert one.p_tile_start(h)[1] == host.p_tile_start(h)[1] == -(-n // h)
            assert (one.p_desc2 is None) == (not two) and one.p_row_off - one.p_desc == host.p_row_off - host.p_desc
            assert (one.total, list(one.offs), one.dt) == (n, [0, n], host.dt)


@pytest.mark.parametrize("with_scores", [True, False], ids=["scores", "mean"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_pool_rows_is_the_three_launches_it_replaced(dtype, with_scores):
    from vlsa_amd import _native as nat
    from vlsa_amd import bag_tables as BT
    from vlsa_amd import functional as VF
    lib, s, p = nat.load(), VF._stream(), VF._p
    g = torch.Generator().manual_seed(7)
    bags = [torch.randn(n, 512, generator=g).to(dtype).to(DEV) for n in [1, 17, 65, 513]]
    B, dt = len(bags), VF._dt(bags[0])
    t = BT.ChunkTables.from_device(BT._stage_table(BT.bag_rows(bags), DEV, "test"), [x.shape[0] for x in bags], dt)
    a = (3.0 * torch.randn(t.total, generator=g)).to(DEV) if with_scores else None
    a_off = t.row_off if with_scores else None
    # the parent's spelling: G, six buffers, the partials, the nine strides, the merge
    G = max(1, min(64, 512 // B))
    pm = torch.empty(B * G, nat.P_STRIDE, dtype=torch.float32, device=DEV)
    pl = torch.empty(B * G, nat.P_STRIDE, dtype=torch.float32, device=DEV)
    pacc = torch.empty(B * G, 512, dtype=torch.float32, device=DEV)
    m2 = torch.empty(B, nat.P_STRIDE, dtype=torch.float32, device=DEV)
    l = torch.empty(B, nat.P_STRIDE, dtype=torch.float32, device=DEV)
    pooled = torch.empty(B, 512, dtype=torch.float32, device=DEV)
    nat.check(lib.vlsa_scored_pool_partial_batch(p(t.desc), B, dt, 512, p(a), p(a_off), G, p(pm), p(pl), p(pacc), s),
              "vlsa_scored_pool_partial_batch")
    st = (ctypes.c_int64 * 9)(nat.P_STRIDE, nat.P_STRIDE, 512, G * nat.P_STRIDE, G * nat.P_STRIDE, G * 512,
                              nat.P_STRIDE, nat.P_STRIDE, 512)
    nat.check(lib.vlsa_vlfan_merge_batch_strided(p(pm), p(pl), p(pacc), B, G, 1, 512, 1, st, p(m2), p(l), p(pooled), s),
              "vlsa_vlfan_merge_batch_strided")
    got, gm2, gl = VF.pool_rows(t.desc, B, dt, a, a_off)
    assert torch.equal(got, pooled)
    assert torch.equal(gm2[:, :1], m2[:, :1]) and torch.equal(gl[:, :1], l[:, :1])       # (P = 1: one entry of each [16] record is written)
    want = torch.stack([(torch.softmax(a[o:o + n], 0)[:, None] * x.float()).sum(0) if with_scores else x.float().mean(0)
                        for x, o, n in zip(bags, t.offs, t.sizes)])
    assert (got - want).abs().max().item() < 1e-4 * max(want.abs().max().item(), 1.0)
