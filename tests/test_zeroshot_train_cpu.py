"""The differentiable zero-shot route (prompt pre-training: identity FeatMIL + logit pooling with trainable text features) without a
GPU: its three entry points are declared and bound, the closed-form gradient its backward kernel implements equals the oracle's
autograd gradient in float64, and every case of the GPU suite meets the selection-gap precondition."""
import ctypes
import re

import numpy as np
import pytest
import torch

import cases
from abi_helpers import HEADER_TEXT
import zeroshot_train_cases as Z
from oracle import vlsa_oracle as O

SYMBOLS = ("vlsa_topk_select_batch", "vlsa_unit_mean_batch", "vlsa_zeroshot_backward_batch")


def test_the_three_entry_points_are_declared_and_bound():
    from vlsa_amd import _native
    for name in SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", HEADER_TEXT), f"{name} is not declared in include/vlsa_hip.h"
        assert name in _native.exported_symbols(), f"{name} is not bound in vlsa_amd/_native.py"
    assert _native._SIGNATURES["vlsa_topk_select_batch"][1][:-2] == _native._SIGNATURES["vlsa_topk_mean_batch"][1][:-1]


@pytest.mark.parametrize("pooling", ["logit_max", "logit_top3", "logit_top10", "logit_mean"])
def test_closed_form_gradient_equals_the_oracles_autograd(pooling):
    sizes, K = (1, 5, 10, 11, 64, 300), 6            # N < k, N == k, N > k
    bags = [cases.make_bag(n, 8500 + i, "iid").double() for i, n in enumerate(sizes)]
    T = torch.randn(K, 512, generator=cases.gen(8600), dtype=torch.float64).requires_grad_(True)
    ls = torch.tensor(cases.LOGIT_SCALE, dtype=torch.float64, requires_grad=True)
    G = torch.randn(len(bags), K, generator=cases.gen(8601), dtype=torch.float64)
    k = Z.topk_of(pooling)
    if k is not None:
        assert Z.min_gap(bags, T.detach(), k) >= Z.GAP
    logits = torch.cat([O.vlsa_zeroshot_forward(X, T, ls, pooling)[0] for X in bags])
    (logits * G).sum().backward()
    got_logits, got_dT, got_dls, idxs = Z.closed_form([X.numpy() for X in bags], T.detach().numpy(), float(ls.detach()), G.numpy(), k)
    assert np.abs(got_logits - logits.detach().numpy()).max() < 1e-10
    assert np.abs(got_dT - T.grad.numpy()).max() < 1e-10 * max(1.0, float(T.grad.abs().max()))
    assert abs(got_dls - float(ls.grad)) < 1e-10 * max(1.0, abs(float(ls.grad)))
    for sel, n in zip(idxs, sizes):
        assert sel.shape == (K, n if k is None else min(k, n))


def test_closed_form_breaks_exact_ties_towards_the_lower_row():
    X = cases.make_bag(12, 8700, "iid").double()
    X = torch.cat([X, X])                              # rows n and n + 12 are equal
    T = torch.randn(3, 512, generator=cases.gen(8701), dtype=torch.float64)
    _, _, _, idxs = Z.closed_form([X.numpy()], T.numpy(), 0.0, np.ones((1, 3)), 4)
    for row in idxs[0]:
        assert row[1] == row[0] + 12 and row[3] == row[2] + 12 and row[0] < 12 and row[2] < 12


@pytest.mark.parametrize("case", [c for c in Z.CASES if Z.topk_of(c[3]) is not None], ids=lambda c: "-".join(map(str, c)))
def test_every_gpu_case_meets_the_selection_gap(case):
    batch, K, dt, pooling = case
    assert Z.min_gap(Z.bags_of(batch, dt), Z.text_of(K, Z.SEEDS[case]), Z.topk_of(pooling)) >= Z.GAP


def test_bad_arguments_are_refused():
    from vlsa_amd import _native as nat
    lib = nat.load()
    one = ctypes.c_void_p(16)
    assert lib.vlsa_topk_select_batch(None, one, 1, 4, 3, None, one, one, None) == -1
    assert lib.vlsa_topk_select_batch(one, one, 1, 4, 3, None, one, None, None) == -1           # k > 0 needs idx
    assert lib.vlsa_topk_select_batch(one, one, 1, 4, 33, None, one, one, None) == -2
    assert lib.vlsa_unit_mean_batch(one, 65, nat.DT_BF16, 512, one, one, None) == -1
    assert lib.vlsa_unit_mean_batch(one, 1, 7, 512, one, one, None) == -1
    assert lib.vlsa_unit_mean_batch(one, 1, nat.DT_BF16, 256, one, one, None) == -2
    args = [one] * 9 + [None]
    assert lib.vlsa_zeroshot_backward_batch(one, 0, nat.DT_BF16, 512, 4, 3, *args) == -1
    assert lib.vlsa_zeroshot_backward_batch(one, 1, nat.DT_BF16, 512, 65, 3, *args) == -1
    assert lib.vlsa_zeroshot_backward_batch(one, 1, nat.DT_BF16, 512, 4, 3, None, *args[1:]) == -1   # k > 0 needs idx
    assert lib.vlsa_zeroshot_backward_batch(one, 1, nat.DT_BF16, 512, 4, 0, one, None, *args[2:]) == -1   # the mean needs u
    assert lib.vlsa_zeroshot_backward_batch(one, 1, nat.DT_BF16, 256, 4, 3, *args) == -2
