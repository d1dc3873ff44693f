"""Torch restatements of DSMIL for the tests: the reference's formula (model/deepmil.py:673-713, written out, not imported) and the
collapsed two-pass form with explicit value-side dropout masks, plus the kernels' counter-based mask generator (vlsa_common.h)."""
import os

import numpy as np
import torch

import dsmil_cases as DC

M32 = 0xFFFFFFFF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _mix(h):
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def dropout_bits(seed, rows, units):
    """vlsa_common.h: dropout_bits(seed, row, unit) for all (row, unit) pairs -> int64 [rows, units]"""
    r = torch.as_tensor(rows, dtype=torch.int64)[:, None]
    u = torch.as_tensor(units, dtype=torch.int64)[None, :]
    return _mix((seed ^ ((r * 0x9E3779B1) & M32) ^ ((u * 0x85EBCA6B) & M32)) & M32)


def bag_seed(s, b):
    """vlsa_common.h: bag_drop_seed"""
    s &= M32
    return s if b == 0 else int(dropout_bits((s ^ 0x5BD1E995) & M32, [b], [M32])[0, 0])


def keep_mask(seed_word, b, n, p):
    """the value-side keep mask [n, 512] of bag b of a launch whose seed word is seed_word"""
    return dropout_bits(bag_seed(int(seed_word), b), range(n), range(512)) >= int(p * 4294967296.0)


def reference_formula(x, P, mask=None, p=0.0):
    """the reference's DSMIL forward on one [N, 512] bag with parameters P = (Wc, bc, Wq, bq, Wv, bv, Wf, bf): (logits [1, C],
    mean-over-classes attention [1, N], critical rows [C]).  mask: keep mask of the value-side dropout (rate p)."""
    Wc, bc, Wq, bq, Wv, bv, Wf, bf = P
    c = x @ Wc.t() + bc
    xd = x if mask is None else x * mask / (1 - p)
    V = xd @ Wv.t() + bv
    Q = x @ Wq.t() + bq
    m = c.argmax(dim=0)
    qmax = x[m] @ Wq.t() + bq
    A = torch.softmax(Q @ qmax.t() / Q.shape[1] ** 0.5, 0)
    Bm = A.t() @ V
    Cc = torch.nn.functional.conv1d(Bm[None], Wf, bf).view(1, -1)
    return 0.5 * (Cc + c.max(dim=0).values), A.detach().mean(dim=1)[None], m


def collapsed_formula(x, P, mask=None, p=0.0):
    """the same function as the kernels evaluate it: C query rows u_k, un-projected weighted sums, projection last"""
    Wc, bc, Wq, bq, Wv, bv, Wf, bf = P
    c = x @ Wc.t() + bc
    m = c.argmax(dim=0)
    qmax = x[m] @ Wq.t() + bq
    u = qmax @ Wq / Wq.shape[0] ** 0.5
    A = torch.softmax(x @ u.t(), 0)
    xd = x if mask is None else x * mask / (1 - p)
    Bm = (A.t() @ xd) @ Wv.t() + bv
    Cc = (Wf * Bm[None]).sum(dim=(1, 2)) + bf
    return 0.5 * (Cc[None] + c.max(dim=0).values), A.detach().mean(dim=1)[None], m


def module_params(m):
    sd = dict(m.named_parameters())
    return [sd[k] for k in DC.KEYS]


def load_case_model(name, device, train=False):
    """(module, rows [N, 512] float32 numpy, fixture) of a fixture case, parameters replayed from the recipe"""
    from vlsa_amd.deepmil import DSMIL
    N, C, rows, seed, sharp, fp = DC.CASES[name]
    fx = np.load(os.path.join(GOLDEN, f"dsmil_{name}.npz"))
    m = DSMIL(dim_in=512, dim_hid=256, num_cls=C, use_feat_proj=fp, drop_rate=0.25)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in DC.make_params(C, seed, fp, float(fx["q_scale"])).items()}, strict=True)
    if fp:
        m.feat_proj.requires_grad_(False)        # the DSMIL backward hands no gradient to the bag rows
    m = m.to(device)
    return (m.train() if train else m.eval()), DC.make_rows(N, rows, seed), fx
