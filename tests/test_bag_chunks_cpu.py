"""vlsa_amd.bag_tables: the helpers every batched model route shares -- ``bag_chunks`` (chunks of <= 64 bags, ILRA's row budget),
``cat`` and ``uniform_bags`` (the non-raising twin of ``checked_bags``).  No GPU: the bags are CPU tensors that say they are on the
device, the set is a stand-in with ``chunk`` / ``sizes``."""
import pytest
import torch

from vlsa_amd import bag_tables as BT
from vlsa_amd._native import VlsaNativeError


class DeviceBag(torch.Tensor):
    """a CPU tensor that answers ``is_cuda`` like a device tensor"""
    is_cuda = True


def bag(n, d=512, dtype=torch.bfloat16, lead=False):
    x = torch.zeros((1, n, d) if lead else (n, d), dtype=dtype)
    return x.as_subclass(DeviceBag)


class FakeSet(list):
    """what ``bag_chunks`` asks of a BagSet: ``chunk(start, n)`` (itself when it covers the set, else a kept sub-set) and ``sizes``"""

    def __init__(self, bags, D=512):
        super().__init__(bags)
        self.D, self.sizes, self.asked = D, tuple(int(x.shape[0]) for x in bags), []

    def chunk(self, start, n):
        self.asked.append((start, n))
        return self if start == 0 and n >= len(self) else FakeSet(list.__getitem__(self, slice(start, start + n)))


COUNTS = {1: [1], 63: [63], 64: [64], 65: [64, 1], 128: [64, 64], 129: [64, 64, 1]}


@pytest.mark.parametrize("count", sorted(COUNTS))
def test_chunks_of_at_most_64(count):
    bags = [bag(1 + i % 3) for i in range(count)]
    for coll in (bags, FakeSet(bags)):
        chunks = list(BT.bag_chunks(coll))
        assert [len(c) for c in chunks] == COUNTS[count]
        flat = [x for c in chunks for x in c]
        assert len(flat) == count and all(a is b for a, b in zip(flat, bags))             # every bag once, in order
        if count <= 64:
            assert chunks[0] is coll                                                      # the object itself, not a copy
        else:
            assert all(type(c) is type(coll) for c in chunks)                             # a set's chunks stay sets
    assert list(BT.bag_chunks([])) == []
    assert [len(c) for c in BT.bag_chunks(bags, n=7)] == [7] * (count // 7) + ([count % 7] if count % 7 else [])


def _ilra_loop(sizes, budget):
    """ILRA.forward_bags' chunking as it stood before ``bag_chunks`` took it over: the (i, j) of every chunk"""
    out, i = [], 0
    while i < len(sizes):
        j, rows = i + 1, sizes[i]
        while j < len(sizes) and j - i < 64 and rows + sizes[j] <= budget:
            rows += sizes[j]
            j += 1
        out.append((i, j))
        i = j
    return out


ROW_CASES = {
    "bigger_than_the_budget": ([10, 250, 10, 10, 300, 300, 5], 100),
    "alone_and_first": ([101, 1], 100),
    "exactly_the_budget": ([40, 60, 40, 60, 100, 99, 1, 1], 100),
    "64_one_row_bags_and_one_more": ([1] * 65, 100),
    "64_one_row_bags_under_a_budget_of_64": ([1] * 65, 64),
    "17_and_65_rows_in_turn": ([17, 65] * 32 + [17], 100),
    "one_bag": ([7], 100),
    "everything_fits": ([3] * 20, 1 << 20),
    "ragged": ([(37 * i) % 90 + 1 for i in range(150)], 128),
}


@pytest.mark.parametrize("case", sorted(ROW_CASES))
def test_row_budget_gives_the_pairs_of_ilras_loop(case):
    sizes, budget = ROW_CASES[case]
    bags = [bag(n) for n in sizes]
    want = _ilra_loop(sizes, budget)
    chunks = list(BT.bag_chunks(bags, 64, budget))
    assert [len(c) for c in chunks] == [j - i for i, j in want]
    assert all(a is b for a, b in zip([x for c in chunks for x in c], bags))
    s = FakeSet(bags)
    set_chunks = list(BT.bag_chunks(s, 64, budget))
    assert s.asked == [(i, j - i) for i, j in want]                                       # sizes from ``sizes``, chunks from ``chunk``
    assert [len(c) for c in set_chunks] == [j - i for i, j in want]
    if len(want) == 1:
        assert chunks[0] is bags and set_chunks[0] is s


def test_cat_returns_the_sole_part_itself():
    a, b = torch.arange(6.0).view(2, 3), torch.ones(1, 3)
    assert BT.cat([a]) is a and BT.cat((a,)) is a
    assert torch.equal(BT.cat([a, b]), torch.cat([a, b]))


MESSAGE = "bags the batched routes do not take"


def _raises(bags):
    try:
        BT.checked_bags(bags, 512, MESSAGE, non_empty=True)
    except (VlsaNativeError, ValueError, AssertionError):
        return True
    return False


TAKEN = {
    "bf16": lambda: [bag(17), bag(65)],
    "fp32": lambda: [bag(17, dtype=torch.float32), bag(1, dtype=torch.float32)],
    "one_bag": lambda: [bag(3)],
    "leading_one": lambda: [bag(17, lead=True), bag(65)],
}
REFUSED = {
    "width_511": lambda: [bag(17), bag(17, 511)],
    "first_of_width_511": lambda: [bag(17, 511)],
    "empty_bag": lambda: [bag(17), bag(0)],
    "mixed_dtypes": lambda: [bag(17), bag(17, dtype=torch.float32)],
    "four_dims": lambda: [bag(17), torch.zeros(1, 1, 17, 512, dtype=torch.bfloat16).as_subclass(DeviceBag)],
    "two_leading": lambda: [torch.zeros(2, 17, 512, dtype=torch.bfloat16).as_subclass(DeviceBag)],
    "cpu_tensor": lambda: [bag(17), torch.zeros(17, 512, dtype=torch.bfloat16)],
}


@pytest.mark.parametrize("case", sorted(TAKEN))
def test_uniform_bags_says_yes_where_checked_bags_passes(case):
    bags = TAKEN[case]()
    assert BT.uniform_bags(bags) and not _raises(bags)
    kept = BT.checked_bags(bags, 512, MESSAGE, non_empty=True)
    assert all(k.dim() == 2 and k.data_ptr() == x.data_ptr() for k, x in zip(kept, bags))        # views of the bags, nothing converted


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_uniform_bags_says_no_where_checked_bags_raises(case):
    bags = REFUSED[case]()
    assert not BT.uniform_bags(bags) and _raises(bags)


def test_fp16_is_converted_by_the_one_and_refused_by_the_other():
    """``checked_bags`` sends every bag through ``_bag2d``, which makes an fp32 copy of an fp16 bag: it serves the COPY.  ``uniform_bags``
    answers for the bags as they are -- its callers launch on them unconverted -- so it cannot say yes."""
    bags = [bag(17, dtype=torch.float16)]
    kept = BT.checked_bags(bags, 512, MESSAGE, non_empty=True)
    assert kept[0].dtype == torch.float32 and kept[0].data_ptr() != bags[0].data_ptr()
    assert not BT.uniform_bags(bags)
    assert BT.uniform_bags(kept)


def test_uniform_bags_of_nothing_and_of_a_set():
    assert not BT.uniform_bags([])
    assert BT.uniform_bags(FakeSet([bag(3)])) and not BT.uniform_bags(FakeSet([bag(3, 256)], D=256))
    assert BT.uniform_bags(FakeSet([bag(3, 256)], D=256), D=256)
