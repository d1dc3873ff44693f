"""A float64 restatement of ILRA (topk = 1, ln = False, eight heads) for the tests, written out from the algebra and not imported from
the reference: eight effective queries per attention block, an un-normalised dot-product softmax pooling, the [1, 256]-sized tail, and
``project_backward`` as a per-row map (it has one key: its softmax is identically 1).  Differentiable in all parameters; the row maps'
ReLU decisions may be GIVEN (the kernel's own).  Also the comparisons every ILRA test applies."""
import math
import os

import numpy as np
import torch

import ilra_cases as IC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-4             # the project's standing tolerance: relative to max(1, max|logits|), to an intermediate's or a gradient's scale


def _lin(x, P, pre, name):
    return x @ P[pre + name + ".weight"].t() + P[pre + name + ".bias"]


def _queries(P, pre, seed):
    Wi, bi = P[pre + "multihead_attn.in_proj_weight"], P[pre + "multihead_attn.in_proj_bias"]
    qf = _lin(seed.view(1, 256), P, pre, "fc_q")[0]
    qp = Wi[:256] @ qf + bi[:256]
    M = Wi[256:512] @ P[pre + "fc_k.weight"]
    return qf, torch.stack([qp[32 * h:32 * h + 32] @ M[32 * h:32 * h + 32] for h in range(8)]) / math.sqrt(32.0)


def _pool(X, E):
    return torch.softmax(X @ E.t(), dim=0).t() @ X                      # [8, d]


def _tail(P, pre, qf, Z, seed, gated, pres):
    Wi, bi = P[pre + "multihead_attn.in_proj_weight"], P[pre + "multihead_attn.in_proj_bias"]
    v = _lin(Z, P, pre, "fc_v") @ Wi[512:].t() + bi[512:]              # [8, 256]
    A = torch.cat([v[h, 32 * h:32 * h + 32] for h in range(8)])
    O = qf + P[pre + "multihead_attn.out_proj.weight"] @ A + P[pre + "multihead_attn.out_proj.bias"]
    t = P[pre + "fc_o.weight"] @ O + P[pre + "fc_o.bias"]
    pres.append(t.detach())
    O = O + torch.relu(t)
    if gated:
        O = O * torch.nn.functional.silu(P[pre + "gate.0.weight"] @ seed.view(256) + P[pre + "gate.0.bias"])
    return O


def forward64(x, P, num_layers, masks=None, dtype=torch.float64):
    """logits [1, num_cls] and the intermediates of one bag x [N, 512] under parameters P (dict by state-dict key, differentiable).
    masks: per block the row map's ReLU decisions [N, 256] bool to take instead of t > 0.  Intermediates: Z{i} [8, d], H{i} [256],
    xhat{i} [N, 256], t{i} [N, 256] (row-map pre-activations), Zp, tail_pre (list of the tails' pre-activations)."""
    P = {k: v.to(dtype) for k, v in P.items()}
    X, out, tails = torch.as_tensor(x).to(dtype), {}, []
    for i in range(num_layers):
        pf, pb = f"gab_blocks.{i}.project_forward.", f"gab_blocks.{i}.project_backward."
        latent = P[f"gab_blocks.{i}.latent"]
        qf, E = _queries(P, pf, latent)
        Z = _pool(X, E)
        H = _tail(P, pf, qf, Z, latent, True, tails)
        c = P[pb + "multihead_attn.out_proj.weight"] @ (P[pb + "multihead_attn.in_proj_weight"][512:] @ _lin(H[None], P, pb, "fc_v")[0]
                                                         + P[pb + "multihead_attn.in_proj_bias"][512:]) + P[pb + "multihead_attn.out_proj.bias"]
        u = X @ P[pb + "fc_q.weight"].t() + (P[pb + "fc_q.bias"] + c)
        t = _lin(u, P, pb, "fc_o")
        m = (t > 0) if masks is None else torch.as_tensor(masks[i])
        o = u + t * m.to(dtype)
        Xh = o * torch.nn.functional.silu(_lin(X, P, pb, "gate.0"))
        out[f"Z{i}"], out[f"H{i}"], out[f"xhat{i}"], out[f"t{i}"] = Z, H, Xh, t.detach()
        X = Xh
    qf, E = _queries(P, "pooling.mha.", P["pooling.S"])
    Zp = _pool(X, E)
    feat = _tail(P, "pooling.mha.", qf, Zp, P["pooling.S"], False, tails)
    out["Zp"], out["tail_pre"] = Zp, tails
    return (feat @ P["classifier.weight"].t() + P["classifier.bias"])[None], out


def run64(x, params, num_layers, w, masks=None):
    """logits, intermediates and the gradients of sum(logits * w) by key, as float64 numpy; params: dict of arrays or tensors"""
    P = {k: torch.as_tensor(v).detach().double().requires_grad_(True) for k, v in params.items()}
    logits, inter = forward64(x, P, num_layers, masks)
    keys = list(P)
    gs = torch.autograd.grad((logits * torch.as_tensor(w).double()).sum(), [P[k] for k in keys], allow_unused=True)
    grads = {k: (torch.zeros_like(P[k]) if g is None else g).numpy() for k, g in zip(keys, gs)}
    inter = {k: (v.detach().numpy() if torch.is_tensor(v) else [t.numpy() for t in v]) for k, v in inter.items()}
    return logits.detach().numpy(), inter, grads


def unpack_mask(words):
    """[N, 8] int32 mask words of the kernel -> [N, 256] bool (bit j of a row = unit j)"""
    w = torch.as_tensor(words).cpu().to(torch.int64) & 0xFFFFFFFF
    return ((w[:, :, None] >> torch.arange(32)) & 1).reshape(w.shape[0], 256).bool()


def load_fixture(name):
    return dict(np.load(os.path.join(GOLDEN, f"ilra_{name}.npz")))


def build_model(num_layers, num_cls, params, device):
    """this package's ILRA with the given parameters"""
    import contextlib
    import io
    from vlsa_amd.deepmil import ILRA
    with contextlib.redirect_stdout(io.StringIO()):
        m = ILRA(dim_in=512, dim_hid=256, num_cls=num_cls, num_layers=num_layers)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in params.items()}, strict=True)
    return m.to(device).eval()


def grad_scale(gmax):
    """per key the scale a gradient error is measured against: the tensor's largest float64 entry; for a tensor whose exact gradient
    is identically zero (project_backward's fc_k and the q / k thirds of its in_proj: one key, the softmax is 1) or rounding noise, a
    relative error does not exist and the case's largest gradient entry is the scale, as the DeepAttnMISL and DSMIL tests do"""
    big = max(gmax.values())
    return {k: (v if v > 1e-9 * big else big) for k, v in gmax.items()}


def check_grads(tag, grads, ref):
    """grads: tensors or arrays by key; ref: float64 arrays by key.  Every tensor within TOL of its scale."""
    scale = grad_scale({k: float(np.abs(ref[k]).max()) for k in ref})
    worst = 0.0
    for k in ref:
        g = grads[k]
        g = g.detach().double().cpu().numpy() if torch.is_tensor(g) else np.asarray(g, dtype=np.float64)
        assert g.shape == ref[k].shape, (tag, k, g.shape, ref[k].shape)
        e = float(np.abs(g - ref[k]).max() / scale[k])
        worst = max(worst, e)
        print(f"[ilra {tag}] d{k}: rel err {e:.2e} (gate {TOL:.0e}, scale {scale[k]:.2e})")
        assert e <= TOL, (tag, k, e)
    return worst


def check_digests(tag, grads, fx, seed, tol):
    """the digests of ``grads`` (float64 arrays by key) against the fixture's, to ``tol`` of the tensor's scale"""
    scale = grad_scale({k: float(fx[f"dg/{k}/gmax"]) for k in grads})
    for k, g in grads.items():
        d = IC.digest(k, g, seed)
        n = np.asarray(g).reshape(-1, np.asarray(g).shape[-1]).shape
        for part, norm in (("gv", math.sqrt(n[1])), ("ug", math.sqrt(n[0])), ("pick", 1.0)):
            e = float(np.abs(d[part] - fx[f"dg/{k}/{part}"]).max() / (scale[k] * norm))
            assert e <= tol, (tag, k, part, e)
        assert abs(float(d["gmax"]) - float(fx[f"dg/{k}/gmax"])) <= tol * scale[k], (tag, k)


def check_mask_band(tag, bits, t64):
    """the kernel's decisions equal t64 > 0 wherever |t64| >= IC.BAND"""
    diff = (np.asarray(bits) != (t64 > 0))
    r, u = np.nonzero(diff)
    worst = float(np.abs(t64[r, u]).max()) if len(r) else 0.0
    print(f"[ilra {tag}] mask: {len(r)} of {diff.size} decisions differ from float64, largest |t64| among them {worst:.2e} (band {IC.BAND:.0e})")
    assert worst < IC.BAND, (tag, len(r), worst)
