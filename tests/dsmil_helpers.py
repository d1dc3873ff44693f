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


def _critical(c, crit):
    """(critical rows, their scores): the argmax over the rows, or the rows ``crit`` names (equal instance scores leave the argmax
    open: a test of the tie rule says which of the equal rows it expects)"""
    if crit is None:
        return c.argmax(dim=0), c.max(dim=0).values
    m = torch.as_tensor(crit, dtype=torch.int64)
    return m, c[m, torch.arange(c.shape[1])]


def reference_formula(x, P, mask=None, p=0.0, crit=None):
    """the reference's DSMIL forward on one [N, 512] bag with parameters P = (Wc, bc, Wq, bq, Wv, bv, Wf, bf): (logits [1, C],
    mean-over-classes attention [1, N], critical rows [C]).  mask: keep mask of the value-side dropout (rate p).  crit: the critical
    rows to take instead of the argmax (see _critical)."""
    Wc, bc, Wq, bq, Wv, bv, Wf, bf = P
    c = x @ Wc.t() + bc
    xd = x if mask is None else x * mask / (1 - p)
    V = xd @ Wv.t() + bv
    Q = x @ Wq.t() + bq
    m, cmax = _critical(c, crit)
    qmax = x[m] @ Wq.t() + bq
    A = torch.softmax(Q @ qmax.t() / Q.shape[1] ** 0.5, 0)
    Bm = A.t() @ V
    Cc = torch.nn.functional.conv1d(Bm[None], Wf, bf).view(1, -1)
    return 0.5 * (Cc + cmax), A.detach().mean(dim=1)[None], m


def collapsed_formula(x, P, mask=None, p=0.0, crit=None):
    """the same function as the kernels evaluate it: C query rows u_k, un-projected weighted sums, projection last"""
    Wc, bc, Wq, bq, Wv, bv, Wf, bf = P
    c = x @ Wc.t() + bc
    m, cmax = _critical(c, crit)
    qmax = x[m] @ Wq.t() + bq
    u = qmax @ Wq / Wq.shape[0] ** 0.5
    A = torch.softmax(x @ u.t(), 0)
    xd = x if mask is None else x * mask / (1 - p)
    Bm = (A.t() @ xd) @ Wv.t() + bv
    Cc = (Wf * Bm[None]).sum(dim=(1, 2)) + bf
    return 0.5 * (Cc[None] + cmax), A.detach().mean(dim=1)[None], m


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


def build_model(C, seed, device, drop=0.25, q_scale=1.0):
    """this package's DSMIL (no Feat_Projecter) with the recipe's parameters make_params(C, seed, q_scale=q_scale), in eval mode"""
    from vlsa_amd.deepmil import DSMIL
    m = DSMIL(dim_in=512, dim_hid=256, num_cls=C, use_feat_proj=False, drop_rate=drop)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in DC.make_params(C, seed, False, q_scale).items()})
    return m.to(device).eval()


# ---- the comparison every DSMIL test applies (test_gpu_dsmil.py against the fixtures, test_gpu_dsmil_edges.py and tools/fuzz_dsmil.py
# against float64 torch): critical rows exact, logits 1e-4 absolute, attention 1e-4 of its largest entry, each gradient
# max(1e-4, 3 x the fp32 error of the same formula in torch) of the tensor's largest float64 entry -------------------------------------
WORST = {"logits": (0.0, 1e-4), "attention": (0.0, 1e-4), "gradient": (0.0, 1e-4)}     # per quantity: the worst (error, its gate) seen


def _note(what, e, tol):
    if e / tol > WORST[what][0] / WORST[what][1]:
        WORST[what] = (e, tol)


def check_grads(tag, grads, ref):
    """grads (in DC.KEYS order) against ref["grad"][k] (float64), scaled by ref["gmax"][k]; ref["referr"][k]: the fp32 error"""
    big = max(float(ref["gmax"][k]) for k in DC.KEYS)
    for k, g in zip(DC.KEYS, grads):
        g = g.double().cpu().numpy()
        assert tuple(g.shape) == tuple(ref["grad"][k].shape), (tag, k, g.shape)
        gmax, referr = float(ref["gmax"][k]), float(ref["referr"][k])
        if gmax == 0.0:           # identically zero in float64 (a one-row bag: the softmax of one score has no gradient):
            gmax = big            # a relative error does not exist; the case's largest gradient entry is the scale
        tol = max(1e-4, 3 * referr)
        e = float(np.abs(g - ref["grad"][k]).max() / gmax)
        print(f"[dsmil {tag}] d{k}: rel err {e:.2e}, gate {tol:.2e}, reference fp32 {referr:.2e}, max|g| {gmax:.2e}")
        _note("gradient", e, tol)
        assert e <= tol, (tag, k, e, tol)


def check_forward(tag, logits, attn, crit, ref):
    assert crit.cpu().tolist() == list(ref["crit"]), (tag, "critical rows", crit.cpu().tolist(), list(ref["crit"]))
    e = float(np.abs(logits.double().cpu().numpy() - ref["logits"]).max())
    print(f"[dsmil {tag}] logits err {e:.2e} (reference fp32 {float(ref['referr']['logits']):.2e})")
    _note("logits", e, 1e-4)
    assert e <= 1e-4, (tag, "logits", e)
    a = attn.double().cpu().numpy()
    assert a.shape == ref["attn"].shape, (tag, a.shape, ref["attn"].shape)
    e = float(np.abs(a - ref["attn"]).max() / np.abs(ref["attn"]).max())
    print(f"[dsmil {tag}] attention rel err {e:.2e} (reference fp32 {float(ref['referr']['attn']):.2e})")
    _note("attention", e, 1e-4)
    assert e <= 1e-4, (tag, "attention", e)


def check_outputs(tag, logits, attn, crit, grads, ref):
    """ref: crit [C], logits [1, C] and attn [1, N] (float64), grad / gmax / referr by key (referr also for "logits" and "attn")"""
    check_forward(tag, logits, attn, crit, ref)
    check_grads(tag, grads, ref)


# ---- float64 (and fp32) torch on the CPU: the reference of the tests that have no fixture ------------------------------------------------
MARGIN = 1e-5        # the top two float64 instance scores of a class must differ by this much, or the critical row is not comparable


def score_margin(x, P, ignore=()):
    """the smallest gap, over the classes, between the largest and the second largest float64 instance score of bag x ([N, 512]);
    ``ignore``: rows left out (the higher copies of a duplicated row: a tie on purpose)"""
    c = x.double() @ P[0].detach().double().t()
    if len(ignore):
        c[list(ignore)] = -float("inf")
    if c.shape[0] - len(ignore) < 2:
        return float("inf")
    top = c.topk(2, dim=0).values
    return float((top[0] - top[1]).min())


def _run(formula, dtype, x, P, cots, crit, mask, p):
    Pd = [t.detach().to(dtype).requires_grad_(True) for t in P]
    logits, attn, m = formula(x.to(dtype), Pd, None if mask is None else mask.to(dtype), p, crit)
    gs = []
    for i, w in enumerate(cots):
        g = torch.autograd.grad((logits * torch.as_tensor(w).to(dtype)).sum(), Pd, retain_graph=i + 1 < len(cots), allow_unused=True)
        gs.append({k: (torch.zeros_like(t) if gi is None else gi).double().numpy() for k, t, gi in zip(DC.KEYS, Pd, g)})
    return logits.detach().double().numpy(), attn.double().numpy(), m.tolist(), gs


def torch_case(x, P, cots, crit=None, formula=reference_formula, mask=None, p=0.0, ignore=()):
    """One bag x ([N, 512] fp32 CPU tensor holding the values the kernels read) through ``formula`` in float64 and in fp32 (both with
    the float64 run's critical rows), with the gradients of sum(logits * w) for every w of ``cots``.  P: the eight parameters (CPU).
    Returns crit, logits, attn, margin, same32 (the fp32 argmax equals the float64 one), grads / grads32 (one dict per w) and the
    fp32 run's errors of logits and attention."""
    lg, at, m, gs = _run(formula, torch.float64, x, P, cots, crit, mask, p)
    lg32, at32, _, gs32 = _run(formula, torch.float32, x, P, cots, m, mask, p)
    with torch.no_grad():
        m32 = (x @ P[0].detach().float().t()).argmax(dim=0).tolist()
    return dict(crit=m, logits=lg, attn=at, margin=score_margin(x, P, ignore), same32=(m32 == m) or crit is not None, grads=gs, grads32=gs32,
                referr={"logits": float(np.abs(lg32 - lg).max()), "attn": float(np.abs(at32 - at).max() / np.abs(at).max())})


def grad_ref(g64, g32):
    """the grad / gmax / referr entries of a check_grads reference from float64 gradients and the fp32 run's"""
    gmax = {k: float(np.abs(g64[k]).max()) for k in DC.KEYS}
    big = max(gmax.values())
    return dict(grad=g64, gmax=gmax, referr={k: float(np.abs(g32[k] - g64[k]).max() / (gmax[k] if gmax[k] > 0 else big)) for k in DC.KEYS})


def case_ref(r, i=0):
    """the check_outputs reference of a torch_case result, for its i-th cotangent"""
    ref = grad_ref(r["grads"][i], r["grads32"][i])
    ref["referr"].update(r["referr"])
    ref.update(crit=r["crit"], logits=r["logits"], attn=r["attn"])
    return ref


def sum_grads(gs):
    return {k: sum(g[k] for g in gs) for k in DC.KEYS}
