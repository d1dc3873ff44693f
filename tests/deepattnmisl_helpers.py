"""A float64 restatement of DeepAttnMISL for the tests (model/deepmil.py:565-580 written out, not imported): the cluster layer as one
product, a ReLU mask that may be GIVEN (the kernel's own decisions), a zero row for an empty cluster, ids outside [0, Kc) in no cluster;
and the comparisons every DeepAttnMISL test applies."""
import os

import numpy as np
import torch

import deepattnmisl_cases as AC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-4             # logits and hc absolute; a gradient relative to the tensor's largest entry (the project's standing tolerance)


def pre64(x, P):
    """pre = Wp x + bp in float64: [N, 256]"""
    return x.double() @ P[0].detach().double().view(256, 512).t() + P[1].detach().double()


def module64(x, ids, P, Kc, mask=None, dtype=torch.float64):
    """(logits [1, num_cls], hc [Kc, 256], pre [N, 256]) of one bag x [N, 512] with cluster ids [N] and the twelve parameters P (in
    AC.KEYS order; differentiable in them).  mask: the ReLU decisions to take ([N, 256] bool) instead of pre > 0."""
    Wp, bp, W0, b0, W1, b1, Ws, bs, W2, b2, Wo, bo = [t.to(dtype) for t in P]
    pre = x.to(dtype) @ Wp.view(256, 512).t() + bp
    m = (pre > 0) if mask is None else mask
    h = pre * m.to(dtype)
    onehot = (torch.as_tensor(ids).long()[:, None] == torch.arange(Kc)[None, :]).to(dtype)        # [N, Kc]: an id outside [0, Kc) selects nothing
    cnt = onehot.sum(dim=0)
    hc = torch.where(cnt[:, None] > 0, (onehot.t() @ h) / cnt.clamp(min=1)[:, None], torch.zeros(Kc, 256, dtype=dtype))
    a = torch.relu(hc @ W0.t() + b0)
    raw = (torch.tanh(a @ W1.t() + b1) * torch.sigmoid(a @ Ws.t() + bs)) @ W2.t() + b2            # [Kc, 1]
    H = torch.softmax(raw.t(), dim=1) @ a
    return H @ Wo.t() + bo, hc, pre


def run64(x, ids, P, Kc, w, mask=None, dtype=torch.float64):
    """logits, hc and the gradients of sum(logits * w) by key, as float64 numpy"""
    Pd = [t.detach().to(dtype).requires_grad_(True) for t in P]
    logits, hc, pre = module64(torch.as_tensor(x), ids, Pd, Kc, mask, dtype)
    gs = torch.autograd.grad((logits * torch.as_tensor(w).to(dtype)).sum(), Pd, allow_unused=True)
    grads = {k: (torch.zeros_like(t) if g is None else g).double().numpy() for k, t, g in zip(AC.KEYS, Pd, gs)}
    return logits.detach().double().numpy(), hc.detach().double().numpy(), pre.detach().double().numpy(), grads


def unpack_mask(words):
    """[N, 8] int32 mask words of the kernel -> [N, 256] bool (bit j of a row = unit j)"""
    w = torch.as_tensor(words).cpu().to(torch.int64) & 0xFFFFFFFF
    return ((w[:, :, None] >> torch.arange(32)) & 1).reshape(w.shape[0], 256).bool()


def load_fixture(name):
    fx = dict(np.load(os.path.join(GOLDEN, f"deepattnmisl_{name}.npz")))
    for k, tag in AC.BIG.items():
        fx["grad/" + k] = np.load(os.path.join(GOLDEN, f"deepattnmisl_{name}_{tag}.npz"))["grad"]
    return fx


def build_model(Kc, num_cls, seed, device, dropout=0.25):
    """this package's DeepAttnMISL with the recipe's parameters, in eval mode"""
    from vlsa_amd.deepmil import DeepAttnMISL
    m = DeepAttnMISL(dim_in=512, dim_hid=256, num_cls=num_cls, num_clusters=Kc, dropout=dropout)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in AC.make_params(Kc, num_cls, seed).items()}, strict=True)
    return m.to(device).eval()


def params_of(m):
    sd = dict(m.named_parameters())
    return [sd[k] for k in AC.KEYS]


def grad_scale(gmax):
    """per key the scale a gradient error is measured against: the tensor's largest float64 entry; for a tensor whose exact gradient is
    identically zero (attention_net.3.fc2.bias: a softmax ignores a common shift of its scores, so its float64 'largest entry' is rounding
    noise) a relative error does not exist and the case's largest gradient entry is the scale, as the DSMIL tests do"""
    big = max(gmax.values())
    return {k: (v if v > 1e-9 * big else big) for k, v in gmax.items()}


def check_grads(tag, grads, ref):
    """grads: tensors in AC.KEYS order; ref: float64 arrays by key"""
    scale = grad_scale({k: float(np.abs(ref[k]).max()) for k in AC.KEYS})
    for k, g in zip(AC.KEYS, grads):
        g = g.detach().double().cpu().numpy()
        assert g.shape == ref[k].shape, (tag, k, g.shape, ref[k].shape)
        e = float(np.abs(g - ref[k]).max() / scale[k])
        print(f"[deepattnmisl {tag}] d{k}: rel err {e:.2e} (gate {TOL:.0e}, max|g| {scale[k]:.2e})")
        assert e <= TOL, (tag, k, e)


def check_mask_band(tag, mask_bits, pre, near=None):
    """the kernel's mask equals pre64 > 0 wherever |pre64| >= BAND; returns whether it equals it EVERYWHERE.  near: the fixture's
    (row, unit) list of |pre64| < 1e-5 -- the disagreeing set must lie inside it."""
    want = torch.as_tensor(pre > 0)
    diff = (mask_bits != want).numpy()
    r, u = np.nonzero(diff)
    worst = float(np.abs(pre[r, u]).max()) if len(r) else 0.0
    print(f"[deepattnmisl {tag}] mask: {len(r)} of {diff.size} decisions differ from float64, largest |pre64| among them {worst:.2e} "
          f"(band {AC.BAND:.0e})")
    assert worst < AC.BAND, (tag, "a ReLU decision outside the band differs", len(r), worst)
    if near is not None:
        assert set(zip(r.tolist(), u.tolist())) <= set(zip(near[0].tolist(), near[1].tolist())), (tag, "disagreement outside the stored list")
    return len(r) == 0
