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


def check_mask_band(tag, bits, t64, band=IC.BAND):
    """the kernel's decisions equal t64 > 0 wherever |t64| >= band (IC.BAND unless the case carries its own)"""
    diff = (np.asarray(bits) != (t64 > 0))
    r, u = np.nonzero(diff)
    worst = float(np.abs(t64[r, u]).max()) if len(r) else 0.0
    print(f"[ilra {tag}] mask: {len(r)} of {diff.size} decisions differ from float64, largest |t64| among them {worst:.2e} (band {band:.1e})")
    assert worst < band, (tag, len(r), worst)


# ---- the entry points alone: inputs, float64 formulas and the measure both GPU files share ------------------------------------------
def rel(tag, got, want, natural=None, gate=TOL):
    """within ``gate`` (TOL) of the largest float64 entry.  natural: the size the terms of the sum have; where the exact result is
    identically zero (one row: the softmax is 1 and dE vanishes) or rounding noise against it, a relative error does not exist and
    ``natural`` is the scale -- the ``grad_scale`` rule above.  Returns the figure."""
    want = np.asarray(want, dtype=np.float64)
    scale = float(np.abs(want).max())
    if natural is not None and scale <= 1e-9 * natural:
        scale = natural
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    e = float(np.abs(got - want).max() / max(scale, 1e-30))
    print(f"[ilra {tag}] rel err {e:.2e} (gate {gate:.1e}, scale {scale:.2e})")
    assert e <= gate, (tag, e)
    WORST[0] = max(WORST[0], e)
    return e


def bag(x, rows, dev):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return (t.bfloat16() if rows == "bf16" else t).contiguous()


def source(N, src, seed, dev):
    """(bags, xp or None, float64 rows [N, D]) of one bag: its own bf16 / fp32 rows (D = 512) or packed fp32 rows ("act", D = 256)"""
    x = IC.make_bag(N, "bf16" if src != "f32" else "f32", seed)
    if src != "act":
        return [bag(x, src, dev)], None, torch.from_numpy(x).double()
    a = (np.random.RandomState(seed + 7).standard_normal((N, 256)) * 0.4).astype(np.float32)
    return [bag(x, "bf16", dev)], torch.from_numpy(a).to(dev), torch.from_numpy(a).double()


WORST = [0.0]          # the largest figure ``rel`` has seen in this process (tools/fuzz_ilra.py reports it)
ROWMAP_KEYS = ("Wq", "btil", "Wo", "bo", "Wg", "bg")


def rowmap_params(rs, D, B=1):
    """the row map's six parameters (fp32 tensors by name) drawn from ``rs``: xavier-sized weights times 2, one b~ row per bag"""
    shp = ((256, D), (B, 256), (256, 256), (256,), (256, D), (256,))
    sc = (2 * np.sqrt(2 / (256 + D)), 0.3, 2 * np.sqrt(1 / 256), 0.05, 2 * np.sqrt(2 / (256 + D)), 0.05)
    return {k: torch.from_numpy((rs.standard_normal(s) * c).astype(np.float32)) for k, s, c in zip(ROWMAP_KEYS, shp, sc)}


def pool_ref(Xs, E, G, dtype=torch.float64):
    """the pooling of a table of bags in ``dtype`` on the CPU: Xs the rows [N_b, D] per bag, E [P, D], G [B, P, D] the weights of the
    loss sum(Z * G).  Z [B, P, D], dE [P, D] (summed over the bags) and dX [sum N_b, D] as float64 arrays."""
    Ed = torch.as_tensor(E).detach().clone().to(dtype).requires_grad_(True)
    Xd = [torch.as_tensor(x).detach().clone().to(dtype).requires_grad_(True) for x in Xs]
    Z = torch.stack([torch.softmax(x @ Ed.t(), dim=0).t() @ x for x in Xd])
    gs = torch.autograd.grad((Z * torch.as_tensor(G).to(dtype)).sum(), [Ed] + Xd)
    return Z.detach().double().numpy(), gs[0].double().numpy(), torch.cat(gs[1:]).double().numpy()


def rowmap_ref(Xs, P, G, bits=None, dtype=torch.float64):
    """the row map of a table of bags in ``dtype`` on the CPU with the ReLU decisions ``bits`` [sum N_b, 256] (None: its own t > 0):
    xhat, t, the decisions taken, the six gradients of sum(xhat * G) by name and dX, as arrays"""
    Pd = {k: torch.as_tensor(P[k]).detach().clone().to(dtype).requires_grad_(True) for k in ROWMAP_KEYS}
    Xd = torch.cat([torch.as_tensor(x).to(dtype) for x in Xs]).requires_grad_(True)
    idx = torch.repeat_interleave(torch.arange(len(Xs)), torch.tensor([int(x.shape[0]) for x in Xs]))
    u = Xd @ Pd["Wq"].t() + Pd["btil"][idx]
    t = u @ Pd["Wo"].t() + Pd["bo"]
    m = (t.detach() > 0) if bits is None else torch.as_tensor(bits).bool()
    o = (u + t * m.to(dtype)) * torch.nn.functional.silu(Xd @ Pd["Wg"].t() + Pd["bg"])
    gs = torch.autograd.grad((o * torch.as_tensor(G).to(dtype)).sum(), [Pd[k] for k in ROWMAP_KEYS] + [Xd])
    grads = {k: g.double().numpy() for k, g in zip(ROWMAP_KEYS, gs)}
    return o.detach().double().numpy(), t.detach().double().numpy(), m.numpy(), grads, gs[-1].double().numpy()


# ---- a case of ilra_edge_cases.py (or a fuzz draw of the same form) on the device and against float64 ---------------------------------
def device_bags(case, inp, dev, stride=None, as_set=False):
    """the bags of a case as device tensors with the case's row stride: a [:, :512] view of an arena whose other columns are NaN"""
    stride = case.stride if stride is None else stride
    out = []
    for x in inp["xs"]:
        t = bag(x, "f32" if case.src == "f32" else "bf16", dev)
        if stride != 512:
            arena = torch.full((t.shape[0], stride), float("nan"), dtype=t.dtype, device=dev)
            arena[:, :512] = t
            t = arena[:, :512]
            assert t.stride(0) == stride or t.shape[0] == 1
        out.append(t)
    if as_set:
        from vlsa_amd.functional import BagSet
        return BagSet(out)
    return out


def _packed(inp, grad, dev):
    return None if inp["a"] is None else torch.from_numpy(inp["a"]).clone().to(dev).requires_grad_(grad)


def run_pool(case, inp, dev="cuda", stride=None, xgrad=None, as_set=False):
    from vlsa_amd import functional as VF
    E = torch.from_numpy(inp["E"]).clone().to(dev).requires_grad_(True)
    xp = _packed(inp, case.xgrad if xgrad is None else xgrad, dev)
    Z = VF.ilra_pool_bags(device_bags(case, inp, dev, stride, as_set), E, xp)
    (Z * torch.from_numpy(inp["G"]).to(dev)).sum().backward()
    return {"Z": Z.detach(), "dE": E.grad, "dX": None if xp is None else xp.grad}


def run_rowmap(case, inp, dev="cuda", stride=None, xgrad=None, as_set=False):
    from vlsa_amd import functional as VF
    Pg = {k: v.detach().clone().to(dev).requires_grad_(True) for k, v in inp["params"].items()}
    xp = _packed(inp, case.xgrad if xgrad is None else xgrad, dev)
    out, mask = VF.ilra_rowmap_bags(device_bags(case, inp, dev, stride, as_set), *[Pg[k] for k in ROWMAP_KEYS], xp, ret_mask=True)
    (out * torch.from_numpy(inp["G"]).to(dev)).sum().backward()
    got = {"xhat": out.detach(), "mask": mask, "dX": None if xp is None else xp.grad}
    got.update({"d" + k: Pg[k].grad for k in ROWMAP_KEYS})
    return got


def run_case(case, inp, **kw):
    return (run_pool if case.kind == "pool" else run_rowmap)(case, inp, **kw)


def _per_bag(case):
    offs = np.concatenate([[0], np.cumsum(case.sizes)])
    return [(b, int(offs[b]), int(offs[b + 1])) for b in range(len(case.sizes))]


def check_pool(case, inp, got):
    """per bag Z, dE summed over the bags and, where the packed rows carry a gradient, dX per bag at its row offset"""
    Z64, dE64, dX64 = pool_ref(inp["rows"], inp["E"], inp["G"])
    rows, G = inp["rows"], inp["G"].astype(np.float64)
    gx = max(float(np.abs(x.astype(np.float64) @ G[b].T).max()) for b, x in enumerate(rows))
    for b, r0, r1 in _per_bag(case):
        rel(f"{case.name} Z[{b}]", got["Z"][b], Z64[b])
    rel(f"{case.name} dE", got["dE"], dE64, natural=gx * max(float(np.abs(x).max()) for x in rows))
    if got["dX"] is not None:
        for b, r0, r1 in _per_bag(case):
            rel(f"{case.name} dX[{b}] rows {r0}..{r1 - 1}", got["dX"][r0:r1], dX64[r0:r1], natural=float(np.abs(G).max()))
    else:
        assert not case.xgrad
    return Z64


def check_rowmap(case, inp, got):
    """the mask within the case's band; xhat, the six gradients (b~ per bag) and dX per bag against float64 under the kernel's mask"""
    bits = unpack_mask(got["mask"]).numpy()
    o64, t64, _, g64, dX64 = rowmap_ref(inp["rows"], inp["params"], inp["G"], bits=bits)
    check_mask_band(case.name, bits, t64, case.band)
    for b, r0, r1 in _per_bag(case):
        rel(f"{case.name} xhat[{b}] rows {r0}..{r1 - 1}", got["xhat"][r0:r1], o64[r0:r1])
    for k in ROWMAP_KEYS:
        if k == "btil":
            for b, _, _ in _per_bag(case):
                rel(f"{case.name} dbtil[{b}]", got["dbtil"][b], g64["btil"][b])
        else:
            rel(f"{case.name} d{k}", got["d" + k], g64[k])
    if got["dX"] is not None:
        for b, r0, r1 in _per_bag(case):
            rel(f"{case.name} dX[{b}] rows {r0}..{r1 - 1}", got["dX"][r0:r1], dX64[r0:r1])
    else:
        assert not case.xgrad


def check_case(case, inp, got):
    return (check_pool if case.kind == "pool" else check_rowmap)(case, inp, got)


def run_module(m, bags, w):
    m.zero_grad(set_to_none=True)
    logits, states = m.forward_bags(bags, ret_state=True)
    (logits * torch.as_tensor(w, device=logits.device)).sum().backward()
    return logits.detach(), states, {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def check_module(tag, logits, states, grads, xs, params, L, w):
    """logits per bag and the gradients of the chunk against the float64 restatement under the kernel's ReLU decisions"""
    assert len(states) == 1
    st, gsum, r0 = states[0], None, 0
    for b, x in enumerate(xs):
        masks = [unpack_mask(st[f"mask{i}"][r0:r0 + len(x)]).numpy() for i in range(L)]
        l64, inter, g = run64(x, params, L, w[b:b + 1], masks=masks)
        for i in range(L):
            check_mask_band(f"{tag} bag {b} block {i}", masks[i], inter[f"t{i}"])          # t of block i under the kernel's earlier decisions
        el, lscale = float(np.abs(logits[b:b + 1].double().cpu().numpy() - l64).max()), max(1.0, float(np.abs(l64).max()))
        print(f"[ilra {tag}] bag {b} N={len(x)}: logits err {el:.2e} (gate {TOL * lscale:.1e})")
        assert el <= TOL * lscale, (tag, b, el)
        gsum = g if gsum is None else {k: gsum[k] + g[k] for k in g}
        r0 += len(x)
    return check_grads(tag + " vs the restatement with the kernel's masks", grads, {k: gsum[k] for k in grads})


def module_fp32_error(xs, params, L, w):
    """the yardstick of a module input: the restatement in plain fp32 torch on the CPU (under float64's ReLU decisions) against float64,
    the worst gradient by ``check_grads``' measure over the sum of the bags -- what fp32 arithmetic itself loses on these inputs"""
    g64 = g32 = None
    for b, x in enumerate(xs):
        _, inter, g = run64(x, params, L, w[b:b + 1])
        P32 = {k: torch.as_tensor(v).detach().float().clone().requires_grad_(True) for k, v in params.items()}
        lg, _ = forward64(x, P32, L, [inter[f"t{i}"] > 0 for i in range(L)], dtype=torch.float32)
        gs = torch.autograd.grad((lg * torch.as_tensor(w[b:b + 1]).float()).sum(), list(P32.values()), allow_unused=True)
        h = {k: (np.zeros_like(g[k]) if t is None else t.double().numpy()) for k, t in zip(P32, gs)}
        g64 = g if g64 is None else {k: g64[k] + g[k] for k in g}
        g32 = h if g32 is None else {k: g32[k] + h[k] for k in h}
    scale = grad_scale({k: float(np.abs(g64[k]).max()) for k in g64})
    return max(float(np.abs(g32[k] - g64[k]).max() / scale[k]) for k in g64)
