"""vlsa_amd.bag_tables on the host alone: the words ``ChunkTables.from_host`` uploads (descriptor rows | second table | row offsets |
int32 tile_start) against an independent restatement, the tables derived by in-stream ops against the packed ones (torch ops on CPU
tensors here), the empty-bag stride rule, the merge strides, and ``score_tile_rows`` against the heights the two earlier copies of
that choice (``FusedAttnScores.pool_bags``, ``AttnBagsPlan``) gave.  No GPU: the bags are stand-ins with an address, a shape and a
stride, and the library's tiling constants are the test's inputs."""
import numpy as np
import pytest
import torch

from vlsa_amd import _native as nat
from vlsa_amd import bag_tables as BT

SIZES = [1, 15, 16, 17, 63, 64, 65, 511, 512, 513, 2798]
HEIGHTS = [16, 32, 64, 128, 256]
BASE = 0x7F3A00000000          # addresses beyond 2^32, as the device hands them out


class FakeBag:
    def __init__(self, ptr, n, stride=512, dtype=torch.bfloat16):
        self._ptr, self.shape, self._stride, self.dtype, self.device = ptr, (n, 512), stride, dtype, torch.device("cpu")

    def data_ptr(self):
        return self._ptr

    def stride(self, i):
        return (self._stride, 1)[i]


def _chunks():
    """B = 1: every size; B = 2: every neighbouring pair; B = 64: the sizes over and over, starting at each of the first three"""
    out = [[n] for n in SIZES] + [[a, b] for a, b in zip(SIZES, SIZES[1:])]
    out += [[SIZES[(i + k) % len(SIZES)] for i in range(64)] for k in range(3)]
    return out


def _bags(sizes, base=BASE):
    bags, p = [], base
    for i, n in enumerate(sizes):
        stride = 512 + 8 * (i % 3)                      # row strides wider than the rows, too
        bags.append(FakeBag(p, n, stride))
        p += (n * stride * 2 + 255) // 256 * 256
    return bags


def _expected_words(bags, second, tile_rows):
    """the upload, word by word, from the layout's description alone"""
    words = []
    for table in (bags, second):
        for x in table or ():
            words += [x.data_ptr(), x.shape[0], x.stride(0)]
    off = 0
    for x in bags:
        words.append(off)
        off += x.shape[0]
    ts = [0]
    for x in bags:
        ts.append(ts[-1] + -(-x.shape[0] // tile_rows))
    lo_hi = ts + [0] * (len(ts) % 2)                    # int32 pairs, little endian, padded to whole words
    words += [lo_hi[i] | (lo_hi[i + 1] << 32) for i in range(0, len(lo_hi), 2)]
    return np.asarray(words, dtype=np.int64), ts, off


@pytest.mark.parametrize("two", [False, True], ids=["one_table", "two_tables"])
@pytest.mark.parametrize("tile_rows", HEIGHTS)
def test_host_constructor_packs_the_documented_words(tile_rows, two):
    for sizes in _chunks():
        bags = _bags(sizes)
        second = [FakeBag(BASE + (1 << 36) + 2048 * sum(sizes[:i]), n, 512, torch.float32) for i, n in enumerate(sizes)] if two else None
        want, ts, total = _expected_words(bags, second, tile_rows)
        t = BT.ChunkTables.from_host(BT.bag_rows(bags), nat.DT_BF16, tile_rows, "cpu", "test", BT.bag_rows(second) if two else None)
        B = len(sizes)
        assert np.array_equal(t.keep.numpy(), want), (sizes, tile_rows)
        # ... and the named pieces are views of exactly those words
        assert t.desc.tolist() == [[x.data_ptr(), x.shape[0], x.stride(0)] for x in bags]
        assert (t.desc2 is None) if not two else t.desc2.tolist() == [[x.data_ptr(), x.shape[0], 512] for x in second]
        assert t.row_off.tolist() == [sum(sizes[:i]) for i in range(B)] and t.row_off.dtype == torch.int64
        got_ts, n_tiles = t.tile_start(tile_rows)
        assert got_ts.dtype == torch.int32 and got_ts.tolist() == ts and n_tiles == ts[-1]
        assert (t.B, list(t.sizes), t.total, t.dt) == (B, sizes, total, nat.DT_BF16) and list(t.offs) == [sum(sizes[:i]) for i in range(B + 1)]
        for p, q in ((t.desc, 0), (t.desc2, 24 * B), (t.row_off, 24 * B * (2 if two else 1)), (got_ts, 24 * B * (2 if two else 1) + 8 * B)):
            assert p is None or p.data_ptr() == t.keep.data_ptr() + q          # the addresses the kernels are handed


@pytest.mark.parametrize("tile_rows", HEIGHTS)
def test_tables_derived_in_stream_equal_the_packed_ones(tile_rows):
    """``from_device`` and a ``tile_start`` of another height than the upload's run torch ops on the descriptor: same values"""
    for sizes in _chunks():
        rows = BT.bag_rows(_bags(sizes))
        host = BT.ChunkTables.from_host(rows, nat.DT_BF16, tile_rows, "cpu", "test")
        dev = BT.ChunkTables.from_device(torch.from_numpy(rows.copy()), tuple(sizes), nat.DT_BF16)
        assert torch.equal(dev.row_off, host.row_off) and dev.total == host.total and list(dev.offs) == list(host.offs)
        for h in HEIGHTS:
            (a, na), (b, nb) = dev.tile_start(h), host.tile_start(h)           # host: h == tile_rows packed, the others derived
            assert a.dtype == b.dtype == torch.int32 and torch.equal(a, b) and na == nb == int(a[-1])
            assert dev.tile_start(h)[0] is a                                    # kept per height
        want = [[BASE + 2048 * sum(sizes[:i]), n, 512] for i, n in enumerate(sizes)]
        assert dev.packed_desc(BASE).tolist() == want


def test_bag_rows_and_the_empty_bag_stride_rule():
    bags = [FakeBag(BASE, 7, 520), FakeBag(BASE + 4096, 0, 0), FakeBag(BASE + 8192, 3, 512)]
    own = BT.bag_rows(bags)
    assert own.dtype == np.int64 and own.tolist() == [[BASE, 7, 520], [BASE + 4096, 0, 0], [BASE + 8192, 3, 512]]
    assert BT.bag_rows(bags, 512).tolist() == [[BASE, 7, 520], [BASE + 4096, 0, 512], [BASE + 8192, 3, 512]]
    assert BT.bag_rows(bags, 512, empty_stride=640).tolist()[1] == [BASE + 4096, 0, 640]
    assert BT.bag_rows([]).shape == (0, 3)


def test_merge_strides():
    S = nat.P_STRIDE
    assert list(BT.merge_strides(8, 12, 512)) == [S, S, 12 * 512, 8 * S, 8 * S, 8 * 12 * 512, S, S, 12 * 512]
    assert list(BT.merge_strides(16, 1, 512)) == [S, S, 512, 16 * S, 16 * S, 16 * 512, S, S, 512]
    rf = 2 * S + 12 * 512
    assert list(BT.merge_strides(4, 12, 512, out=(rf, rf, rf))) == [S, S, 12 * 512, 4 * S, 4 * S, 4 * 12 * 512, rf, rf, rf]


# (max_rows, round_tiles) of vlsa_gated_scores_tiling and (big_rows, big_min) of vlsa_gated_scores_big_tile per (fp32, gated), as the
# library answers with no VLSA_GS_* switch set
TILING = {(False, False): (128, 256, 256, 1), (False, True): (64, 64, 256, 1), (True, False): (128, 256, 0, 0), (True, True): (64, 64, 0, 0)}
CASES = {"large": [50000, 1, 24000, 12000], "b32": [2798] * 32, "one17": [17]}
# (case, gated, fp32) -> rows per tile of AttnBagsPlan, (rows per tile, one-launch route) of pool_bags, the same under VLSA_GS_NO_FUSED_POOL=1
RECORDED = {
    ("large", True, True): (64, (64, False), (64, False)), ("large", True, False): (256, (256, True), (64, False)),
    ("large", False, True): (128, (128, False), (128, False)), ("large", False, False): (256, (256, True), (128, False)),
    ("b32", True, True): (64, (64, False), (64, False)), ("b32", True, False): (256, (256, True), (64, False)),
    ("b32", False, True): (128, (128, False), (128, False)), ("b32", False, False): (256, (256, True), (128, False)),
    ("one17", True, True): (16, (16, False), (16, False)), ("one17", True, False): (96, (96, True), (16, False)),
    ("one17", False, True): (16, (16, False), (16, False)), ("one17", False, False): (160, (160, True), (16, False)),
}


@pytest.mark.parametrize("case,gated,f32", sorted(RECORDED))
def test_score_tile_rows_gives_what_both_earlier_copies_gave(case, gated, f32):
    from vlsa_amd.functional import score_tile_rows
    plan_rpt, pool, pool_no_fused = RECORDED[(case, gated, f32)]
    tiling = TILING[(f32, gated)]
    assert score_tile_rows(CASES[case], f32, gated, True, tiling=tiling)[0] == plan_rpt
    assert score_tile_rows(CASES[case], f32, gated, True, tiling=tiling) == pool
    assert score_tile_rows(CASES[case], f32, gated, False, tiling=tiling) == pool_no_fused
