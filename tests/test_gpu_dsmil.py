"""DSMIL on the GPU (vlsa_amd.deepmil.DSMIL over vlsa_dsmil_forward_batch / _backward_batch) against the reference's own DSMIL in
float64 (tests/golden/dsmil_*.npz, make_golden_dsmil.py): critical rows, logits, attention and every parameter gradient, through
``forward`` and through ``forward_bags`` with all fixtures' bags in one ragged batch; batch == single calls bit for bit; run-to-run
reproducibility; the value-side dropout (masks, gradients, fresh masks per step); a short Adam run and its captured-graph replay.

Gates: logits 1e-4 absolute, attention 1e-4 of its largest entry, each gradient max(1e-4, 3 x the reference's own fp32 error) of the
tensor's largest float64 entry (the project's standing 1e-4; the reference's fp32 run is itself up to 8.6e-4 off at 50k rows).  The
two [256, 512] gradients are compared whole, from files of their own (float64 rounded to float32: 6e-8 of an entry).  A gradient that is identically
zero in float64 (b_classifier.q.* of a one-row bag) has no relative error: it is measured against the case's largest gradient entry.  The comparison
itself is dsmil_helpers.check_outputs, shared with test_gpu_dsmil_edges.py.  Equal instance scores cannot be tested against the reference (its
torch.sort leaves ties open); that the kernels take the lowest row -- in the per-lane scan, the 16-way merge of a part and the merge of the
parts -- is tested in test_gpu_dsmil_edges.py (test_equal_scores_resolve_to_the_lowest_row, test_a_bag_of_identical_rows) against the
float64 formula evaluated at the expected row."""
import os

import numpy as np
import pytest
import torch

import dsmil_cases as DC
import dsmil_helpers as DH

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _rows_dtype(name):
    return torch.float32 if DC.CASES[name][2] == "f32" else torch.bfloat16


def _check_case(name, fx, logits, attn, crit, grads, how):
    """the fixture as a reference of the shared comparison (dsmil_helpers.check_outputs)"""
    big = {k: np.load(os.path.join(DH.GOLDEN, f"dsmil_{name}_{tag}.npz"))["grad"].astype(np.float64) for k, tag in DC.BIG.items()}
    for k, g in zip(DC.KEYS, grads):
        assert tuple(g.shape) == tuple(fx["shape/" + k])
    referr = {k: float(fx["referr/" + k]) for k in DC.KEYS}
    referr.update(logits=float(fx["referr/logits"]), attn=float(fx["referr/attn"]))
    ref = dict(crit=fx["crit"].tolist(), logits=fx["logits"], attn=fx["attn"].astype(np.float64), referr=referr,
               grad={k: big[k] if k in DC.BIG else fx["grad/" + k] for k in DC.KEYS}, gmax={k: float(fx["gmax/" + k]) for k in DC.KEYS})
    DH.check_outputs(f"{name} {how}", logits, attn, crit, grads, ref)


@pytest.mark.parametrize("name", list(DC.CASES))
def test_forward_matches_the_reference_in_float64(name):
    m, x, fx = DH.load_case_model(name, DEV)
    X = torch.from_numpy(x).to(_rows_dtype(name)).to(DEV)[None]
    logits, attn, crit = m(X, ret_with_attn=True, ret_critical=True)
    assert tuple(logits.shape) == (1, DC.CASES[name][1]) and tuple(attn.shape) == (1, x.shape[0])
    (logits * torch.from_numpy(DC.make_w(DC.CASES[name][1], DC.CASES[name][3])).to(DEV)).sum().backward()
    _check_case(name, fx, logits.detach(), attn, crit[0], [p.grad for p in DH.module_params(m)], "forward")
    assert torch.equal(m(X), logits.detach())                       # without the extras: the same logits, [1, C]


@pytest.fixture(scope="module")
def all_rows():
    return {n: DC.make_rows(c[0], c[2], c[3]) for n, c in DC.CASES.items()}


@pytest.mark.parametrize("name", list(DC.CASES))
def test_forward_bags_matches_the_reference_with_all_fixture_bags_in_one_batch(name, all_rows):
    from vlsa_amd import functional as VF
    m, _, fx = DH.load_case_model(name, DEV)
    dt = _rows_dtype(name)
    names = list(DC.CASES)
    bags = [torch.from_numpy(all_rows[n]).to(dt).to(DEV) for n in names]      # 1 .. 50 000 rows, ragged
    i = names.index(name)
    logits, attn, crit = m.forward_bags(VF.BagSet(bags), ret_with_attn=True, ret_critical=True)
    assert tuple(logits.shape) == (len(bags), DC.CASES[name][1]) and [a.shape[1] for a in attn] == [b.shape[0] for b in bags]
    w = torch.from_numpy(DC.make_w(DC.CASES[name][1], DC.CASES[name][3])).to(DEV)
    (logits[i:i + 1] * w).sum().backward()
    _check_case(name, fx, logits[i:i + 1].detach(), attn[i], crit[i], [p.grad for p in DH.module_params(m)], "forward_bags")


def _synthetic(sizes, dtype, seed):
    return [torch.from_numpy(DC.make_rows(n, "bf16", seed + i)).to(dtype).to(DEV) for i, n in enumerate(sizes)]


def _model(C=4, drop=0.25, seed=5, q_scale=8.0):
    from vlsa_amd.deepmil import DSMIL
    m = DSMIL(dim_in=512, dim_hid=256, num_cls=C, use_feat_proj=False, drop_rate=drop)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in DC.make_params(C, seed, False, q_scale).items()})
    return m.to(DEV)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_a_batch_equals_single_calls_bit_for_bit(dtype):
    m = _model(C=5).eval()
    bags = _synthetic([1, 17, 513, 2798, 700, 6000, 64, 33000], dtype, 100)
    G = torch.randn(len(bags), 5, generator=torch.Generator().manual_seed(1)).to(DEV)
    logits, attn = m.forward_bags(bags, ret_with_attn=True)
    (logits * G).sum().backward()
    gb = [p.grad.clone() for p in DH.module_params(m)]
    m.zero_grad(set_to_none=True)
    singles = [m(x[None], ret_with_attn=True) for x in bags]
    for i, (lg, a) in enumerate(singles):
        assert torch.equal(lg[0], logits[i]) and torch.equal(a, attn[i]), i
    # the gradient of bag i alone through the batch (the other bags' dlogits zero) equals the single call's, bit for bit
    for i in (0, 3, 7):
        m.zero_grad(set_to_none=True)
        (singles[i][0] * G[i:i + 1]).sum().backward()
        gs = [p.grad.clone() for p in DH.module_params(m)]
        m.zero_grad(set_to_none=True)
        Gi = torch.zeros_like(G)
        Gi[i] = G[i]
        (m.forward_bags(bags) * Gi).sum().backward()
        for a, b, k in zip(gs, DH.module_params(m), DC.KEYS):
            assert torch.equal(a, b.grad), (i, k)
    assert all(torch.isfinite(g).all() for g in gb)


def test_two_runs_of_a_training_step_give_identical_gradients():
    from vlsa_amd import functional as VF
    bags = VF.BagSet(_synthetic([2798, 300, 9000, 1, 4100], torch.bfloat16, 200))
    G = torch.randn(5, 4, generator=torch.Generator().manual_seed(2)).to(DEV)
    runs = []
    for _ in range(2):
        m = _model().train()
        m._drop_counter = torch.tensor([4321], dtype=torch.int64, device=DEV)
        (m.forward_bags(bags) * G).sum().backward()
        runs.append([p.grad.clone() for p in DH.module_params(m)])
    for a, b, k in zip(runs[0], runs[1], DC.KEYS):
        assert torch.equal(a, b), k


@pytest.mark.parametrize("dtype,C", [(torch.float32, 4), (torch.bfloat16, 6), (torch.bfloat16, 12)])
def test_dropout_masks_and_gradients_match_torch_on_the_collapsed_formula_with_the_same_masks(dtype, C):
    """training mode: the kernels' masks are dropout_bits(bag_drop_seed(seed, b), row, feature) >= p 2^32 -- restated in Python and
    fed to torch autograd on the collapsed formula (float64)"""
    from vlsa_amd import functional as VF
    p, s = 0.25, 777001
    m = _model(C=C).train()
    bags = _synthetic([900, 2798, 17, 1], dtype, 300)
    G = torch.randn(len(bags), C, generator=torch.Generator().manual_seed(3)).to(DEV)
    m._drop_counter = torch.tensor([s - 1], dtype=torch.int64, device=DEV)     # the call advances it to s
    logits = m.forward_bags(VF.BagSet(bags))
    (logits * G).sum().backward()
    P64 = [t.detach().double().cpu().requires_grad_(True) for t in DH.module_params(m)]
    ref = torch.cat([DH.collapsed_formula(x.double().cpu(), P64, DH.keep_mask(s, b, x.shape[0], p).double(), p)[0] for b, x in enumerate(bags)])
    (ref * G.double().cpu()).sum().backward()
    e = (logits.detach().double().cpu() - ref.detach()).abs().max().item()
    print(f"[dsmil dropout {dtype} C={C}] logits err {e:.2e}")
    assert e <= 1e-4
    # without the masks the result is visibly different: the masks are really applied
    plain = torch.cat([DH.collapsed_formula(x.double().cpu(), [t.detach() for t in P64])[0] for x in bags[:2]])
    assert (plain - ref.detach()[:2]).abs().max().item() > 1e-5     # (the masked run agrees to ~1e-8)
    for k, t, r in zip(DC.KEYS, DH.module_params(m), P64):
        e = (t.grad.double().cpu() - r.grad).abs().max().item() / r.grad.abs().max().item()
        print(f"[dsmil dropout {dtype} C={C}] d{k}: rel err {e:.2e}")
        assert e <= 1e-4, (k, e)


def test_two_consecutive_steps_draw_different_masks_and_eval_draws_none():
    m = _model().train()
    bags = _synthetic([2798, 500], torch.bfloat16, 400)
    with torch.no_grad():
        a, b = m.forward_bags(bags), m.forward_bags(bags)
        assert (a - b).abs().max().item() > 1e-5
        m.eval()
        assert torch.equal(m.forward_bags(bags), m.forward_bags(bags))


def _adam_run(bags, t, e, steps, hip, graph=False):
    """Adam on SurvIFMLE(softmax(logits)); hip: this package's DSMIL (eval-mode dropout), else torch on the reference formula"""
    from vlsa_amd.losses import SurvIFMLE
    loss_fn = SurvIFMLE()
    m = _model(drop=0.0).train()
    params = DH.module_params(m)
    opt = torch.optim.Adam(params, lr=1e-3, capturable=True)

    def step():
        opt.zero_grad(set_to_none=False)
        if hip:
            logits = m.forward_bags(bags)
        else:
            logits = torch.cat([DH.reference_formula(x.float(), params)[0] for x in bags])
        loss = loss_fn(torch.softmax(logits, dim=1), t, e)
        loss.backward()
        opt.step()
        return loss.detach()
    losses = []
    if graph:
        for p in params:
            p.grad = torch.zeros_like(p)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                  # warm-up outside the capture, then back to the starting point
            start = [p.detach().clone() for p in params]
            step()
            with torch.no_grad():
                for p, s0 in zip(params, start):
                    p.copy_(s0)
                for st in opt.state.values():
                    for v in st.values():
                        if torch.is_tensor(v):
                            v.zero_()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = step()
        for _ in range(steps):
            g.replay()
            losses.append(float(out))
    else:
        losses = [float(step()) for _ in range(steps)]
    return losses, [p.detach().clone() for p in params]


def test_three_adam_steps_lower_the_loss_match_torch_and_replay_from_a_captured_graph():
    from vlsa_amd import functional as VF
    bags = VF.BagSet(_synthetic([300 + 411 * i for i in range(8)], torch.bfloat16, 500))
    bags.desc()
    t = torch.tensor([0, 1, 2, 3, 0, 1, 2, 3], device=DEV)
    e = torch.tensor([1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0], device=DEV)
    lh, ph = _adam_run(bags, t, e, 3, hip=True)
    lt, pt = _adam_run(bags, t, e, 3, hip=False)
    print(f"[dsmil adam] hip losses {lh}, torch losses {lt}")
    assert lh[2] < lh[0]
    for a, b in zip(lh, lt):
        assert abs(a - b) <= 1e-4
    for k, a, b in zip(DC.KEYS, ph, pt):
        err = (a - b).abs().max().item()
        print(f"[dsmil adam] {k}: max param diff {err:.2e} of {b.abs().max().item():.2e}")
        assert err <= 1e-4 * b.abs().max().item(), k
    lg, pg = _adam_run(bags, t, e, 3, hip=True, graph=True)
    assert lg == lh, (lh, lg)                        # the replays reproduce the eager steps: same kernels, same order, same bits
    for k, a, b in zip(DC.KEYS, ph, pg):
        assert torch.equal(a, b), (k, (a - b).abs().max().item())


def test_a_bag_that_requires_grad_and_a_trainable_projecter_are_refused():
    from vlsa_amd._native import VlsaNativeError
    from vlsa_amd.deepmil import DSMIL
    m = _model().eval()
    x = _synthetic([64], torch.float32, 600)[0].requires_grad_(True)
    with pytest.raises(VlsaNativeError, match="requires grad"):
        m(x[None])
    mp = DSMIL(dim_in=512, dim_hid=256, num_cls=4, use_feat_proj=True).to(DEV)
    with pytest.raises(VlsaNativeError, match="freeze feat_proj"):
        mp(x.detach()[None])
    with torch.no_grad():
        assert tuple(mp(x.detach()[None]).shape) == (1, 4)
