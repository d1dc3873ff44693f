"""The batched max / mean pooling kernels (vlsa_colmax_batch, vlsa_pool_dx_batch, vlsa_gather_rows_batch through VF.max_pool_bags,
VF.mean_pool_bags and VF.gather_rows_bags) on the bags of tests/maxpool_cases.py: values and FIRST maximal rows against torch's CPU
``max`` (exact, ties included), a bag alone against the same bag among ragged neighbours (bit-equal), the dense row gradients of both
poolings, their layout as views of one buffer, and the gather of the selected rows."""
import pytest
import torch

import maxpool_cases as MC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = [torch.bfloat16, torch.float32]
_DEVICE_BAGS, _ALONE = {}, {}


def _P():
    from vlsa_amd import _native
    return int(_native.load().vlsa_colmax_part_rows())


def _bags(dtype):
    """{name: (device bag, (values, rows) on the CPU)}; ``strided`` stays a row-stride-640 view"""
    if dtype not in _DEVICE_BAGS:
        out = {}
        for name, (x, ref) in MC.build(_P(), dtype).items():
            xd = x._base.to(DEV)[:, :512] if name == "strided" else x.to(DEV)
            assert xd.stride() == x.stride()
            out[name] = (xd, ref)
        _DEVICE_BAGS[dtype] = out
    return _DEVICE_BAGS[dtype]


def _alone(dtype):
    """every bag pooled in a call of its own: {name: (out [512], idx [512])} on the CPU"""
    from vlsa_amd import functional as VF
    if dtype not in _ALONE:
        res = {}
        for name, (x, _) in _bags(dtype).items():
            out, idx = VF.max_pool_bags([x], return_index=True)
            assert out.shape == idx.shape == (1, 512) and out.dtype == torch.float32 and idx.dtype == torch.int32
            res[name] = (out[0].cpu(), idx[0].cpu())
        _ALONE[dtype] = res
    return _ALONE[dtype]


def _batches(names, B):
    """B == 3: every window of three neighbours (each bag is seen first, in the middle and last); B == 64: the cases cycled to 64 bags
    from two starting points"""
    k = len(names)
    if B == 3:
        return [[names[(i + j) % k] for j in range(3)] for i in range(k)]
    return [[names[(s + j) % k] for j in range(64)] for s in (0, 5)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_bag_per_call_equals_torch_max_values_and_first_rows(dtype):
    for name, (out, idx) in _alone(dtype).items():
        v, i = _bags(dtype)[name][1]
        assert torch.equal(out, v), name
        assert torch.equal(idx, i), (name, (idx != i).nonzero().flatten().tolist()[:8])


@pytest.mark.parametrize("B", [3, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_batch_equals_torch_max_and_the_bags_alone_bit_for_bit(dtype, B):
    from vlsa_amd import functional as VF
    bags, alone = _bags(dtype), _alone(dtype)
    for k, batch in enumerate(_batches(list(bags), B)):
        chunk = [bags[n][0] for n in batch]
        out, idx = VF.max_pool_bags(VF.BagSet(chunk) if k % 2 else chunk, return_index=True)
        out, idx = out.cpu(), idx.cpu()
        for b, n in enumerate(batch):
            v, i = bags[n][1]
            assert torch.equal(out[b], v) and torch.equal(idx[b], i), (n, b)
            assert torch.equal(out[b].view(torch.int32), alone[n][0].view(torch.int32)), (n, b)      # the same bits, -0.0 included
            assert torch.equal(idx[b], alone[n][1]), (n, b)


def _leaves(dtype, names):
    """fresh leaves that require grad; for ``strided`` the leaf is the [N, 640] base and the bag its [:, :512] view"""
    leaves, bags = [], []
    for n in names:
        x = _bags(dtype)[n][0]
        leaf = (x._base if n == "strided" else x).detach().clone().requires_grad_(True)
        leaves.append(leaf)
        bags.append(leaf[:, :512] if n == "strided" else leaf)
    return leaves, bags


@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_row_gradients_of_max_and_mean_and_their_layout(dtype, B):
    """max: the one-hot scatter of dpooled to the first maximal rows, bit for bit (in the bag's dtype).  mean: dpooled / N in every row
    within one fp32 ulp of the float64 quotient (bf16 bags: that, rounded to bf16).  Both: the per-bag gradients arrive as views of
    one packed fp32 buffer, bag b at byte 2048 * (rows before it)."""
    from vlsa_amd import functional as VF
    names = list(_bags(dtype))
    names = (["slide_2798"] if B == 1 else names[4:7] if B == 3 else [names[(3 + j) % len(names)] for j in range(64)])
    G = torch.randn(len(names), 512, generator=torch.Generator().manual_seed(B)).to(DEV)
    for pool in (VF.max_pool_bags, VF.mean_pool_bags):
        leaves, bags = _leaves(dtype, names)
        seen = {}
        for b, x in enumerate(bags):
            x.register_hook(lambda g, b=b: seen.__setitem__(b, (g.data_ptr(), g.dtype, tuple(g.shape), g.is_contiguous())))
        out = pool(bags)
        assert out.requires_grad and out.shape == (len(names), 512)
        (out * G).sum().backward()
        offs, o = [], 0
        for x in bags:
            offs.append(o)
            o += x.shape[0]
        if dtype == torch.float32:               # (bf16 bags get a cast copy of their slice)
            assert all(seen[b] == (seen[0][0] + 2048 * offs[b], torch.float32, tuple(bags[b].shape), True) for b in range(len(bags)))
        for b, (n, leaf) in enumerate(zip(names, leaves)):
            g = leaf.grad[:, :512].cpu()
            assert g.dtype == dtype
            if n == "strided":
                assert (leaf.grad[:, 512:] == 0).all()
            N, Gb = g.shape[0], G[b].cpu()
            if pool is VF.max_pool_bags:
                ref = torch.zeros(N, 512)
                ref[_bags(dtype)[n][1][1].long(), torch.arange(512)] = Gb
                assert torch.equal(g, ref.to(dtype)), (n, b)
            else:
                ref = (Gb.double() / N)[None, :].expand(N, 512)
                r32 = ref.float().abs()
                tol = (torch.nextafter(r32, torch.full_like(r32, float("inf"))) - r32).double()
                if dtype == torch.bfloat16:
                    tol = tol + ref.abs() * 2.0 ** -8            # one more rounding, to 8 significant bits
                assert ((g.double() - ref).abs() <= tol).all(), (n, b, (g.double() - ref).abs().max().item())
                assert (g == g[0:1]).all()                        # the same value in every row


@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_rows_equals_indexing(dtype, B):
    from vlsa_amd import _native, functional as VF
    bags = _bags(dtype)
    names = [list(bags)[(2 + 3 * j) % len(bags)] for j in range(B)]
    chunk = VF.BagSet([bags[n][0] for n in names])
    idx = torch.stack([bags[n][1][1] for n in names]).to(DEV)
    got = VF.gather_rows_bags(chunk.desc(), B, _native.DT_F32 if dtype == torch.float32 else _native.DT_BF16, idx)
    assert got.shape == (B * 512, 512) and got.dtype == torch.float32
    ref = torch.cat([bags[n][0].float()[bags[n][1][1].long().to(DEV)] for n in names])
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_mean_pool_without_grad_keeps_its_bits_and_takes_a_bagset_table():
    from vlsa_amd import _native, functional as VF
    chunk = [x for x, _ in list(_bags(torch.bfloat16).values())[:7]]
    ref = VF.pool_rows(VF._stage_table(VF.bag_rows(chunk), DEV, "test"), len(chunk), _native.DT_BF16, None, None)[0]
    assert torch.equal(VF.mean_pool_bags(chunk), ref) and torch.equal(VF.mean_pool_bags(VF.BagSet(chunk)), ref)
