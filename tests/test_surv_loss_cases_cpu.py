"""CPU side of the survival loss kernel tests: the float64 truth of tests/surv_loss_cases.py is tied to the pinned helpers, every case's
inputs keep the conditions that make a float64 comparison meaningful, and the two gates the GPU tests apply are measured here as 8 x the
worst error of a plain fp32 evaluation of the same formulas."""
import functools
import math

import numpy as np
import pytest
import torch

import cases
import surv_eval_helpers as H
import surv_loss_cases as C
from oracle import vlsa_oracle as O

INCIDENCE_FIXTURES = [n for n in H.fixture_names() if n.endswith("_incidence")]


def test_dispatch_constants_match_the_library():
    from vlsa_amd import _native as nat
    assert C.MAX_K == nat.MAX_K and C.ROWS16_MAX_K < C.MAX_K
    assert C.LOG_LOGIT_SCALE == cases.LOGIT_SCALE


@pytest.mark.parametrize("name", INCIDENCE_FIXTURES)
def test_per_sample_forms_have_the_pinned_means(name):
    fx = H.load_fixture(name)
    ext = H.fixture_ext(fx) or dict(logit_scale=C.LOGIT_SCALE, alpha=0.0, eps=1e-7, p=2, raw_distance=True)
    y = H.convert(fx["raw"], "incidence")
    for alpha in (0.0, 0.3, ext["alpha"]):
        want = H.loss_mle(y, fx["t"], fx["e"], "incidence", alpha, ext["eps"])
        got = C.truth(y, fx["t"], fx["e"], ext["logit_scale"], alpha, ext["eps"], from_logits=False).ifmle
        assert got.dtype == torch.float64 and got.shape == (len(fx["t"]),)
        assert abs(float(got.mean()) - want) <= 1e-14 * abs(want)
    for p, raw in [(2, True), (2, False), (1, True), (ext["p"], ext["raw_distance"])]:
        want = H.loss_emd(y, fx["t"], fx["e"], ext["logit_scale"], p, raw)
        rows = H.loss_emd_rows(y, fx["t"], fx["e"], ext["logit_scale"], p, raw)
        got = C.truth(y, fx["t"], fx["e"], ext["logit_scale"], p=p, raw_distance=raw, from_logits=False).emd
        assert rows.dtype == torch.float64 and rows.shape == (len(fx["t"]),) and torch.equal(rows, got)
        assert abs(float(rows.mean()) - want) <= 1e-14 * abs(want)


def test_truth_objective_and_gradient_are_those_of_the_weighted_mean():
    i = C.make_inputs(33, 12, 5, 2.0)
    r = C.truth(i.logits, i.t, i.e, C.LOGIT_SCALE, alpha=0.3, w_ifmle=0.5, w_emd=2.0)
    assert float(r.objective) == float((0.5 * r.ifmle + 2.0 * r.emd).mean())
    x = i.logits.double()
    h = 1e-4            # truncation ~ h^2 = 1e-8, rounding ~ 1e-16 / h = 1e-12
    for (row, col) in [(0, 0), (1, 10), (7, 3), (32, 11)]:      # central differences of the float64 objective
        d = torch.zeros_like(x)
        d[row, col] = h
        up = C.truth(x + d, i.t, i.e, C.LOGIT_SCALE, alpha=0.3, w_ifmle=0.5, w_emd=2.0).objective
        dn = C.truth(x - d, i.t, i.e, C.LOGIT_SCALE, alpha=0.3, w_ifmle=0.5, w_emd=2.0).objective
        assert abs(float(up - dn) / (2 * h) - float(r.grad[row, col])) <= 1e-6 * float(r.grad.abs().max())


def test_case_tables_hold_what_the_kernels_branch_on():
    assert len(C.GRID) == 50 and len(C.BIG) == 6 and len(C.EXTREME) == 3 and len(C.OPTIONS) == 96
    assert len({c.name for c in C.OBJECTIVE_CASES}) == len(C.OBJECTIVE_CASES)
    ks = {c.K for c in C.GRID}
    assert {1, C.ROWS16_MAX_K - 1, C.ROWS16_MAX_K, C.ROWS16_MAX_K + 1, C.MAX_K - 1, C.MAX_K} <= ks
    assert {1, C.CHUNK - 1, C.CHUNK, C.CHUNK + 1} <= {c.B for c in C.GRID}
    assert {c.B for c in C.BIG} == {C.ONE_BLOCK_MAX_B - 1, C.ONE_BLOCK_MAX_B, C.ONE_BLOCK_MAX_B + 1}
    assert all(c.all_events == (c.p == 2 and not c.raw) for c in C.OBJECTIVE_CASES)


@pytest.mark.parametrize("c", C.OBJECTIVE_CASES, ids=C.ids(C.OBJECTIVE_CASES))
def test_inputs_keep_their_conditions(c):
    i = C.case_inputs(c)
    _check_inputs(i.logits, i.t, i.e, i.changed, c.B, c.K, c.all_events, c.p, C.LOGIT_SCALE)


@pytest.mark.parametrize("K,B", C.ROW_SHAPES)
def test_per_sample_inputs_keep_their_conditions(K, B):
    i = C.make_inputs(B, K, 7000 + 100 * K + B, 2.0)
    inc, t, e = C.row_inputs(K, B)
    assert torch.equal(inc, torch.softmax(i.logits, dim=-1)) and torch.equal(e, i.e)
    _check_inputs(i.logits, t, e, i.changed, B, K, False, 2, C.ROW_LOGIT_SCALE)


def _check_inputs(logits, t, e, changed, B, K, all_events, p, ls):
    assert logits.shape == (B, K) and logits.dtype == torch.float32 and t.dtype == torch.int64 and e.dtype == torch.float32
    assert int(t.min()) >= 0 and int(t.max()) < K
    inc = torch.softmax(logits.double(), dim=-1)
    cen = e == 0
    if K >= 15:
        assert changed <= 0.25 * B, changed
    if K >= 2 and B >= 31 and not all_events:
        assert int(cen.sum()) >= 5 and int((~cen).sum()) >= 5, (int(cen.sum()), int((~cen).sum()))
    if K >= 2:
        tail = 1.0 - torch.cumsum(inc, dim=-1).gather(1, t.view(-1, 1)).view(-1)
        assert bool((tail[cen] >= C.MIN_TAIL).all())
    if B >= 4 and not all_events:
        assert t[:4].tolist() == [0, max(K - 2, 0), K - 1, 0] and e[0] == 1 and e[2] == 1       # (the tail rule may claim samples 1 and 3)
    # the clamp of an event's inc[t] at eps, and with it the -1 / a gradient, switches at 1e-7
    a = inc.gather(1, t.view(-1, 1)).view(-1)[~cen]
    assert not bool(((a >= 0.5e-7) & (a <= 2e-7)).any())
    if p == 1:
        # |d| has a kink at 0: no cdf difference of a bin below the last may sit within fp32 rounding of it.  (The last bin's difference
        # is zero up to rounding by construction; its sign adds one constant to every suffix sum and to their weighted mean and cancels.)
        # Checked on the events.  A censored sample's differences are ALL zero up to rounding at this logit scale -- prediction and
        # target both spread evenly over the bins >= t -- and its whole EMD gradient is bounded by 2 K e^-ls whatever the signs are:
        assert 2 * K * math.exp(-ls) < 1e-20
        y = torch.softmax(logits, dim=-1)
        k = torch.arange(K).view(1, K)
        target = ((k == t.view(-1, 1)).long() + (k > t.view(-1, 1)).long() * (1 - e.view(-1, 1).long())).double()
        pred = torch.where(cen.view(-1, 1), (1 - target) * y.double() + target * ls, y.double())
        d = torch.cumsum(torch.softmax(pred, dim=-1), dim=-1) - torch.cumsum(torch.softmax((2 * target - 1) * ls, dim=-1), dim=-1)
        assert float(d[~cen][:, :K - 1].abs().min()) >= 1e-6


@functools.lru_cache(maxsize=None)
def _objective_errors(c):
    want, got = C.case_truth(c), C.case_truth(c, torch.float32)
    ev, eg = C.rel_value(got.objective, want.objective), C.rel_grad(got.grad, want.grad)
    if (c.p, c.raw, c.alpha, c.w_ifmle, c.w_emd) == (2, True, 0.0, 1.0, 1.0):      # ... and the oracle the existing loss tests compare with
        i = C.case_inputs(c)
        x = i.logits.clone().requires_grad_(True)
        o = O.vlsa_objective(x, i.t, i.e, torch.tensor(C.LOG_LOGIT_SCALE).exp())
        o.backward()
        ev, eg = max(ev, C.rel_value(o.detach(), want.objective)), max(eg, C.rel_grad(x.grad, want.grad))
    return ev, eg


@functools.lru_cache(maxsize=None)
def _row_errors(K, B, which):
    (v64, g64), (v32, g32) = C.row_truth(K, B, which), C.row_truth(K, B, which, torch.float32)
    return C.rel_value_rows(v32, v64), C.rel_grad_rows(g32, g64)


@pytest.mark.parametrize("c", C.OBJECTIVE_CASES, ids=C.ids(C.OBJECTIVE_CASES))
def test_fp32_restatement_of_the_objective_stays_within_an_eighth_of_the_gates(c):
    ev, eg = _objective_errors(c)
    print(f"{c.name}: fp32 restatement value {ev:.2e} (gate {C.VALUE_RTOL:g}) gradient {eg:.2e} (gate {C.GRAD_RTOL:g})")
    assert ev <= C.VALUE_RTOL / 8 and eg <= C.GRAD_RTOL / 8


@pytest.mark.parametrize("which", ["ifmle", "emd"])
@pytest.mark.parametrize("K,B", C.ROW_SHAPES)
def test_fp32_restatement_of_the_per_sample_route_stays_within_an_eighth_of_the_gates(K, B, which):
    ev, eg = _row_errors(K, B, which)
    print(f"rows {which} K={K} B={B}: fp32 restatement values {ev:.2e} (gate {C.ROW_VALUE_RTOL:g}) gradient rows {eg:.2e} (gate {C.GRAD_RTOL:g})")
    assert ev <= C.ROW_VALUE_RTOL / 8 and eg <= C.GRAD_RTOL / 8


def _round_up_one_digit(v):
    m = 10.0 ** math.floor(math.log10(v))
    return math.ceil(v / m - 1e-9) * m


def test_gates_are_eight_times_the_fp32_restatement():
    """the gates of surv_loss_cases.py are 8 x the worst figure over every case, rounded up to one significant digit -- no tighter (a
    correct fp32 kernel reaches them) and no looser"""
    worst = {}
    for kind, err, where in ([("value", _objective_errors(c)[0], c.name) for c in C.OBJECTIVE_CASES] +
                             [("gradient", _objective_errors(c)[1], c.name) for c in C.OBJECTIVE_CASES] +
                             [(f"{q} of the per-sample route", _row_errors(K, B, w)[j], f"{w} K={K} B={B}")
                              for K, B in C.ROW_SHAPES for w in ("ifmle", "emd") for j, q in enumerate(("values", "gradient rows"))]):
        if err > worst.get(kind, (-1.0, ""))[0]:
            worst[kind] = (err, where)
    for kind, (err, where) in worst.items():
        print(f"worst fp32 restatement error, {kind}: {err:.3e} at {where}")
    value, row_value = 8 * worst["value"][0], 8 * worst["values of the per-sample route"][0]
    grad = 8 * max(worst["gradient"][0], worst["gradient rows of the per-sample route"][0])
    print(f"gates: VALUE_RTOL {_round_up_one_digit(value):g} (8 x worst = {value:.2e}), GRAD_RTOL {_round_up_one_digit(grad):g} (8 x worst = {grad:.2e}), "
          f"ROW_VALUE_RTOL {_round_up_one_digit(row_value):g} (8 x worst = {row_value:.2e})")
    assert math.isclose(C.ROW_VALUE_RTOL, _round_up_one_digit(row_value), rel_tol=1e-9)
    assert math.isclose(C.VALUE_RTOL, _round_up_one_digit(value), rel_tol=1e-9)
    assert math.isclose(C.GRAD_RTOL, _round_up_one_digit(grad), rel_tol=1e-9)


def test_pair_counts_blocked_equals_pair_counts():
    g = np.random.default_rng(300)
    time, event = g.integers(0, 6, 300).astype(np.float64), g.random(300) < 0.6
    est = g.choice(np.linspace(-1.0, 1.0, 8), 300)
    est[:40] += g.normal(size=40) * 1e-8            # some pairs inside, some outside the tie tolerance
    want = H.pair_counts(time, event, est)
    assert want[2] > 0 and want[3] > 0
    for rows in (512, 256, 7, 1):
        assert H.pair_counts_blocked(time, event, est, rows=rows) == want
