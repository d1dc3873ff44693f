"""The head and tail kernels of vlsa_amd/csrc/vlfan_tail.hip and the merge-and-pool kernels of vlsa_amd/csrc/vlfan_batch.hip on every
dispatch path -- ticketed / rows route, MFMA / VALU adapter, `pre` / in-place finish, fused / unfused single-slide tail, small / batch
merge-pool, the backward's chunks, the query chain -- against float64 references (tests/head_path_cases.py).  Every test prints its
figure next to its gate before it asserts; the worst figure per entry point is printed when the module is done.

Then: routes that must agree (bit for bit where the code promises it), ticket reuse, the host refusals, and VLSA.forward /
_deepmil_logits for DeepMIL encoders of width 256 and 768 against the torch-ops fallback evaluated in float64."""
import ctypes
import functools
import math

import pytest
import torch

import head_path_cases as HC

pytestmark = pytest.mark.gpu
WORST = {}            # entry -> (figure in units of its gate, output, case id)
SENT = 7.25e3         # fills what a kernel must not write
TICKET_SENT = 0x5A5A5A5A


def _dev():
    return torch.device("cuda", 0)


def _lib():
    from vlsa_amd import _native as nat, functional as F
    return nat.load(), nat, F


class _Outs:
    """output buffers with 64 guard floats behind each: ``check`` asserts that nothing wrote past an output"""

    def __init__(self):
        self.bufs = []

    def new(self, *shape):
        n = math.prod(shape)
        buf = torch.full((n + 64,), SENT, dtype=torch.float32, device=_dev())
        self.bufs.append((buf, n))
        return buf[:n].view(*shape)

    def check(self):
        torch.cuda.synchronize()
        for buf, n in self.bufs:
            assert bool((buf[n:] == SENT).all()), "a kernel wrote past an output buffer"


def _up(t):
    return None if t is None else t.contiguous().to(_dev())


def _judge(c, got, ref):
    """print every output's error next to its gate, keep the worst per entry, then assert"""
    bad = []
    for label, e, g in HC.judged(c, got, ref):
        ratio = HC.ratio(e, g)
        print(f"[head paths] {c.id} {'/'.join(HC.case_path(c))} {label}: {e:.3e} (gate {g:.1e})")
        if c.entry not in WORST or not ratio <= WORST[c.entry][0]:
            WORST[c.entry] = (ratio, label, c.id)
        if not ratio <= 1.0:
            bad.append((label, e, g))
    assert not bad, (c.id, bad)


@pytest.fixture(scope="module", autouse=True)
def _worst_figures():
    """after the module's tests: the worst figure per entry point among the cases that ran, in units of its gate"""
    yield
    for entry, (r, label, cid) in sorted(WORST.items()):
        print(f"\n[head paths] worst {entry:17s}: {r:.3f} of its gate ({label}) at {cid}", end="")
    print(f"\n[head paths] cases: { {e: len(HC.cases_of(e)) for e in HC.ENTRIES} }")


# ---- one runner per entry point ---------------------------------------------------------------------------------------------------------
def _head_forward(c, inp):
    lib, nat, F = _lib()
    h = F.head_forward(_up(inp["rows"][0]), c.mode, _up(inp["pw"]), _up(inp["W"]), _up(inp["b"]), _up(inp["That"]), _up(inp["ls"]),
                       want_incidence=c.inc)
    torch.cuda.synchronize()
    return {k: v for k, v in h.items() if v is not None}


def _head_args(c, inp, o):
    B, P, D, K = c.B, c.P, c.D, c.K
    out = dict(pooled=o.new(B, D), v=o.new(B, D), vhat=o.new(B, D), vnorm=o.new(B), logits=o.new(B, K))
    if c.inc:
        out["incidence"] = o.new(B, K)
    return out


def _head_batch(c, inp, counters=None, text=False):
    lib, nat, F = _lib()
    p, o = F._p, _Outs()
    B, P, D, K = c.B, c.P, c.D, c.K
    rows, W, b, pw, ls = _up(inp["rows"]), _up(inp["W"]), _up(inp["b"]), _up(inp["pw"]), _up(inp["ls"])
    text_rows = _up(inp["T"] if text else inp["That"])      # (held in a name: a temporary would be freed before the launch)
    out = _head_args(c, inp, o)
    if c.layout == "inplace":
        out["pooled"] = rows.view(B, D)
    tail = (p(out["pooled"]), p(out["v"]), p(out["vhat"]), p(out["vnorm"]), p(out["logits"]), p(out.get("incidence")), F._stream())
    if text:
        out["That"], out["tnorm"] = o.new(K, D), o.new(K)
        nat.check(lib.vlsa_head_forward_batch_text(p(rows), B, P, D, HC.POOL_CODE[c.mode], p(pw), p(W), p(b), p(text_rows), K, p(ls),
                                                   p(out["That"]), p(out["tnorm"]), *tail), "vlsa_head_forward_batch_text")
    else:
        rows_route = HC.case_path(c)[0] == "rows"
        if counters is None:         # the rows route must not touch the tickets; the ticketed one needs them zeroed and hands them back so
            counters = torch.full((B,), TICKET_SENT if rows_route else 0, dtype=torch.int32, device=_dev())
        before = counters.clone()
        nat.check(lib.vlsa_head_forward_batch(p(rows), B, P, D, HC.POOL_CODE[c.mode], p(pw), p(W), p(b), p(text_rows), K, p(ls),
                                              p(counters), *tail), "vlsa_head_forward_batch")
        torch.cuda.synchronize()
        assert torch.equal(counters, before) if rows_route else int(counters.abs().max()) == 0, "ticket words"
    o.check()
    return out


def _merge_inputs(c, inp):
    """pm / pl with NaN in the columns p >= P (no kernel may read them), pacc as it is"""
    pm, pl = inp["pm"].clone(), inp["pl"].clone()
    pm[..., c.P:] = float("nan")
    pl[..., c.P:] = float("nan")
    return pm, pl, inp["pacc"]


def _merge_head(c, inp, fused=True):
    """vlsa_vlfan_merge_head; fused = False: vlsa_vlfan_merge + vlsa_head_forward, the route the entry takes when it cannot fuse"""
    lib, nat, F = _lib()
    p, o = F._p, _Outs()
    G, P, D, K = c.G, c.P, c.D, c.K
    pm, pl, pacc = (_up(t[0]) for t in _merge_inputs(c, inp))
    W, b, pw, ls, That = _up(inp["W"]), _up(inp["b"]), _up(inp["pw"]), _up(inp["ls"]), _up(inp["That"])
    ws = torch.zeros(lib.vlsa_head_workspace_bytes(D), dtype=torch.uint8, device=_dev())
    out = dict(m2=o.new(16), l=o.new(16), out=o.new(P, D), pooled=o.new(D), v=o.new(D), vhat=o.new(D), vnorm=o.new(1), logits=o.new(K))
    if c.inc:
        out["incidence"] = o.new(K)
    head = (p(out["pooled"]), p(out["v"]), p(out["vhat"]), p(out["vnorm"]), p(out["logits"]), p(out.get("incidence")), F._stream())
    code = HC.POOL_CODE[c.mode]
    if fused:
        nat.check(lib.vlsa_vlfan_merge_head(p(pm), p(pl), p(pacc), G, P, D, code, p(pw), p(W), p(b), p(That), K, p(ls), p(ws), p(out["m2"]),
                                            p(out["l"]), p(out["out"]), *head), "vlsa_vlfan_merge_head")
    else:
        nat.check(lib.vlsa_vlfan_merge(p(pm), p(pl), p(pacc), G, P, D, 1, p(out["m2"]), p(out["l"]), p(out["out"]), F._stream()), "vlsa_vlfan_merge")
        nat.check(lib.vlsa_head_forward(p(out["out"]), P, D, code, p(pw), p(W), p(b), p(That), K, p(ls), p(ws), *head), "vlsa_head_forward")
    o.check()
    assert int(ws[:256].max()) == 0, "the ticket words of the workspace are handed back zeroed"
    out["m2"], out["l"] = out["m2"][:P], out["l"][:P]
    return out


def _merge_head_batch(c, inp, strides=None):
    lib, nat, F = _lib()
    p, o = F._p, _Outs()
    B, G, P, D, K = c.B, c.G, c.P, c.D, c.K
    st = strides or HC.strided_layout(c)
    sm, sl, sa, bm, bl, ba, om, ol, oo = st
    pm, pl, pacc = _merge_inputs(c, inp)

    def place(t, rec, bag, width):          # [B, G, width] -> a NaN-filled buffer with the record and bag strides
        buf = torch.full((B * bag + 16,), float("nan"), dtype=torch.float32)
        torch.as_strided(buf, (B, G, width), (bag, rec, 1)).copy_(t.reshape(B, G, width))
        return buf.to(_dev())

    dpm, dpl, dpa = place(pm, sm, bm, 16), place(pl, sl, bl, 16), place(pacc, sa, ba, P * D)
    m2, l, out_ = o.new(B * om), o.new(B * ol), o.new(B * oo)
    W, b, pw, ls, That = _up(inp["W"]), _up(inp["b"]), _up(inp["pw"]), _up(inp["ls"]), _up(inp["That"])
    out = _head_args(c, inp, o)
    nat.check(lib.vlsa_vlfan_merge_head_batch_strided(p(dpm), p(dpl), p(dpa), B, G, P, D, (ctypes.c_int64 * 9)(*st), HC.POOL_CODE[c.mode], p(pw),
                                                      p(W), p(b), p(That), K, p(ls), p(m2), p(l), p(out_), p(out["pooled"]), p(out["v"]),
                                                      p(out["vhat"]), p(out["vnorm"]), p(out["logits"]), p(out.get("incidence")), F._stream()),
              "vlsa_vlfan_merge_head_batch_strided")
    o.check()
    for buf, bag, width in ((m2, om, P), (l, ol, P), (out_, oo, P * D)):      # the spare floats between the bags' outputs stay untouched
        spare = torch.ones(B * bag, dtype=torch.bool, device=_dev())
        torch.as_strided(spare, (B, width), (bag, 1)).fill_(False)
        assert bool((buf[spare] == SENT).all()), "a merge kernel wrote between two bags' outputs"
    out.update(m2=torch.as_strided(m2, (B, P), (om, 1)), l=torch.as_strided(l, (B, P), (ol, 1)),
               out=torch.as_strided(out_, (B, P, D), (oo, D, 1)))
    return out


def _head_backward(c, inp):
    lib, nat, F = _lib()
    p, o = F._p, _Outs()
    B, P, D, K = c.B, c.P, c.D, c.K
    sv = {k: _up(v) for k, v in HC.backward_saved(c, inp).items()}
    W, dl, gv, gt, ls = _up(inp["W"]), _up(inp["dlogits"]), _up(inp["g_vhat"]), _up(inp["g_That"]), _up(inp["ls"])
    ws = o.new(B * D + B)
    out = dict(drows=o.new(B, P, D), dT=o.new(K, D), dls=o.new(1))
    if W is not None:
        out.update(dW=o.new(D, D), db=o.new(D))
    nat.check(lib.vlsa_head_backward_batch(p(dl), p(gv), p(gt), p(sv["pooled"]), p(sv["vhat"]),
                                           p(sv["vnorm"]), p(sv["That"]), p(sv["tnorm"]), p(sv["logits"]), p(W), p(ls), B, P, D, K,
                                           p(ws), p(out["drows"]), p(out.get("dW")), p(out.get("db")), p(out["dT"]), p(out["dls"]), F._stream()),
              "vlsa_head_backward_batch")
    o.check()
    return out


def _head_train(c, inp):
    lib, nat, F = _lib()
    leaf = lambda t: None if t is None else _up(t).requires_grad_(True)  # noqa: E731
    rows, W, b, T, ls = leaf(inp["rows"]), leaf(inp["W"]), leaf(inp["b"]), leaf(inp["T"]), leaf(inp["ls"])
    logits, vhat, That = F.head_train(rows, W, b, T, ls, F.HeadTickets())
    ((logits * _up(inp["dlogits"])).sum() + (vhat * _up(inp["g_vhat"])).sum() + (That * _up(inp["g_That"])).sum()).backward()
    torch.cuda.synchronize()
    out = dict(logits=logits.detach(), vhat=vhat.detach(), That=That.detach(), drows=rows.grad, dT=T.grad, dls=ls.grad)
    if W is not None:
        out.update(dW=W.grad, db=b.grad)
    return out


def _qprep_block(c, inp):
    """the prepared-query block vlsa_query_chain reads q^ and max(|q|, 1e-12) from: vlsa_prepare_queries where it takes the width
    (D % 8 == 0, at most 16 effective queries), else the same block filled in by hand (float64 values rounded to fp32) through PreparedQueries' own views"""
    lib, nat, F = _lib()
    Q = inp["Q"]
    if c.D % 8 == 0 and c.P <= HC.MAX_P:
        return F.prepare_queries(_up(Q), c.gated)
    qp = F.PreparedQueries(torch.zeros(lib.vlsa_qprep_bytes(c.D), dtype=torch.uint8, device=_dev()), c.nq, c.P, c.D, c.gated)
    n = Q.double().norm(dim=-1).clamp_min(HC.NORM_EPS)
    qp.qhat.copy_((Q.double() / n[:, None]).float())
    qp.qnorm.copy_(n.float())
    return qp


def _query_chain(c, inp):
    lib, nat, F = _lib()
    o = _Outs()
    qp = _qprep_block(c, inp)
    dQ, dE = o.new(c.nq, c.D), _up(inp["dE"])
    nat.check(lib.vlsa_query_chain(F._p(dE), F._p(qp.buf), c.nq, int(c.gated), c.D, F._p(dQ), F._stream()), "vlsa_query_chain")
    o.check()
    return {"dQ": dQ}


RUN = {"head_forward": _head_forward, "head_batch": _head_batch, "head_batch_text": functools.partial(_head_batch, text=True),
       "merge_head": _merge_head, "merge_head_batch": _merge_head_batch, "head_backward": _head_backward, "head_train": _head_train,
       "query_chain": _query_chain}


@pytest.mark.parametrize("c", HC.CASES, ids=[c.id for c in HC.CASES])
def test_case_against_float64(c):
    inp = HC.make_inputs(c)
    _judge(c, RUN[c.entry](c, inp), HC.reference(c, inp))


@pytest.mark.parametrize("D", HC.WIDTHS)
def test_normalize_rows_against_float64(D):
    """VF.normalize_rows (the unit text rows every forward entry is handed) at every width: rows of norm 3 sqrt(D), 1e3, 1e-6 and zero"""
    lib, nat, F = _lib()
    T = torch.randn(7, D, generator=torch.Generator().manual_seed(D)) * 3
    T[1] *= 1e3
    T[2] *= 1e-6
    T[3] = 0.0
    That, tnorm = F.normalize_rows(_up(T))
    n = T.double().norm(dim=-1).clamp_min(HC.NORM_EPS)
    e, en = HC.err_of(That.cpu(), T.double() / n[:, None]), HC.err_of(tnorm.cpu(), n)
    print(f"[head paths] normalize_rows-D{D} That: {e:.3e} (gate {HC.GATE_THAT:.1e})  tnorm: {en:.3e} (gate {HC.GATE_ROWS * float(n.max()):.1e})")
    assert e <= HC.GATE_THAT and en <= HC.GATE_ROWS * float(n.max())


# ---- routes that must agree -----------------------------------------------------------------------------------------------------------
def _within_gates(c, a, b, what):
    """two routes of the library on the same inputs: each output of ``a`` within the case's gate of ``b`` (the gates of the float64 test)"""
    for label, e, g in HC.judged(c, a, {k: v.detach().double().cpu() for k, v in b.items()}):
        print(f"[head paths] {what} {c.id} {label}: {e:.3e} (gate {g:.1e})")
        assert e <= g, (what, c.id, label, e, g)


@pytest.mark.parametrize("B,P,D,K,mode,adapter", [(9, 12, 252, 4, "mean", True), (17, 2, 768, 17, "weight", True), (17, 12, 512, 16, "max", True),
                                                   (33, 1, 1020, 64, "mean", False), (2, 16, 4, 1, "max", True)])
def test_text_route_equals_normalize_plus_batch_bit_for_bit(B, P, D, K, mode, adapter):
    """vlsa_head_forward_batch_text = vlsa_normalize_rows + vlsa_head_forward_batch at widths other than 512 too: the same kernels on the
    same values, so every output agrees bit for bit"""
    lib, nat, F = _lib()
    c = HC.Case("head_batch_text", B=B, P=P, D=D, K=K, mode=mode, adapter=adapter)
    inp = HC.make_inputs(c)
    fused = _head_batch(c, inp, text=True)
    That, tnorm = F.normalize_rows(_up(inp["T"]))
    two = _head_batch(HC.Case("head_batch", B=B, P=P, D=D, K=K, mode=mode, adapter=adapter), dict(inp, That=That.cpu()))
    two.update(That=That, tnorm=tnorm)
    for name in fused:
        assert torch.equal(fused[name], two[name]), name


@pytest.mark.parametrize("G,P,K,mode", [(1, 1, 1, "mean"), (17, 12, 4, "weight"), (257, 16, 64, "mean"), (512, 2, 17, "weight")])
def test_fused_single_slide_tail_agrees_with_the_unfused_route(G, P, K, mode):
    c = HC.Case("merge_head", G=G, P=P, K=K, mode=mode)
    assert HC.case_path(c)[0] == "fused"
    inp = HC.make_inputs(c)
    _within_gates(c, _merge_head(c, inp, fused=True), _merge_head(c, inp, fused=False), "fused vs unfused")


@pytest.mark.parametrize("B", [16, 17, 33])
def test_mfma_adapter_agrees_with_the_valu_adapter(B):
    """the same bags through k_head_linear_mfma (B >= 16 at D = 512) and, nine at a time, through k_head_linear"""
    c = HC.Case("head_batch", B=B, P=2, D=512, K=4, mode="mean")
    assert "mfma" in HC.case_path(c)
    inp = HC.make_inputs(c)
    whole = _head_batch(c, inp)
    parts = []
    for b0 in range(0, B, 9):
        n = min(9, B - b0)
        cs = HC.Case("head_batch", B=n, P=2, D=512, K=4, mode="mean")
        assert n > 1 and "valu" in HC.case_path(cs)
        parts.append(_head_batch(cs, dict(inp, rows=inp["rows"][b0:b0 + n])))
    pieces = {k: torch.cat([p_[k] for p_ in parts]) for k in whole}
    _within_gates(c, whole, pieces, "mfma vs valu")


@pytest.mark.parametrize("P,D,mode,layout", [(12, 512, "mean", "contig"), (1, 516, "max", "strided"), (16, 252, "weight", "strided"), (5, 768, "max", "contig")])
def test_small_merge_pool_agrees_with_the_batch_kernel(P, D, mode, layout):
    """G = 8 records through k_vlfan_merge_pool_small, then the same records and a ninth, empty one through k_vlfan_merge_pool_batch"""
    c8 = HC.Case("merge_head_batch", B=3, G=8, P=P, D=D, K=4, mode=mode, layout=layout)
    c9 = HC.Case("merge_head_batch", B=3, G=9, P=P, D=D, K=4, mode=mode, layout=layout)
    assert HC.case_path(c8)[0] == "small" and HC.case_path(c9)[0] == "batch"
    inp = HC.make_inputs(c8)
    empty = lambda t, fill: torch.cat([t, torch.full_like(t[:, :1], fill)], dim=1)  # noqa: E731
    inp9 = dict(inp, pm=empty(inp["pm"], float("-inf")), pl=empty(inp["pl"], 0.0), pacc=empty(inp["pacc"], 0.0))
    _within_gates(c8, _merge_head_batch(c9, inp9), _merge_head_batch(c8, inp), "batch vs small merge-pool")


# ---- tickets ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,adapter", [(512, True), (508, True), (1024, False)])
def test_head_forward_reuses_its_workspace(D, adapter):
    """three vlsa_head_forward calls back to back on ONE workspace: the same bits each time, the ticket words zero afterwards"""
    lib, nat, F = _lib()
    p = F._p
    c = HC.Case("head_forward", P=12, D=D, K=4, adapter=adapter)
    inp = HC.make_inputs(c)
    rows, W, b, That, ls = _up(inp["rows"][0]), _up(inp["W"]), _up(inp["b"]), _up(inp["That"]), _up(inp["ls"])
    ws = torch.zeros(lib.vlsa_head_workspace_bytes(D), dtype=torch.uint8, device=_dev())
    runs = []
    for _ in range(3):
        o = _Outs()
        out = [o.new(D), o.new(D), o.new(D), o.new(1), o.new(4), o.new(4)]
        nat.check(lib.vlsa_head_forward(p(rows), 12, D, 0, None, p(W), p(b), p(That), 4, p(ls), p(ws), *(p(t) for t in out), F._stream()), "head")
        runs.append(out)
    torch.cuda.synchronize()
    assert int(ws[:256].max()) == 0
    for out in runs[1:]:
        assert all(torch.equal(a, b_) for a, b_ in zip(runs[0], out))
    ref = HC.reference(c, inp)
    assert HC.err_of(runs[2][4].cpu(), ref["logits"]) <= HC.GATE_LOGITS


@pytest.mark.parametrize("B,D,adapter", [(1, 512, True), (5, 512, True), (5, 516, True), (5, 768, False)])
def test_batched_ticketed_head_reuses_its_counters(B, D, adapter):
    """three vlsa_head_forward_batch calls (given pooling: the grid (NB, B)) on ONE counter buffer: same bits, counters zero afterwards"""
    c = HC.Case("head_batch", B=B, P=1, D=D, K=4, mode="given", adapter=adapter)
    assert HC.case_path(c)[0] == "ticketed"
    inp = HC.make_inputs(c)
    counters = torch.zeros(B, dtype=torch.int32, device=_dev())
    runs = [_head_batch(c, inp, counters=counters) for _ in range(3)]
    assert int(counters.abs().max()) == 0
    for out in runs[1:]:
        assert all(torch.equal(runs[0][k], out[k]) for k in out)
    _judge(c, runs[2], HC.reference(c, inp))


def test_rows_route_leaves_the_counters_alone():
    c = HC.Case("head_batch", B=5, P=12, D=516, K=4)
    assert HC.case_path(c)[0] == "rows"
    counters = torch.full((5,), TICKET_SENT, dtype=torch.int32, device=_dev())
    _head_batch(c, HC.make_inputs(c), counters=counters)
    assert bool((counters == TICKET_SENT).all())


# ---- refusals: VLSA_EINVAL before anything is launched ------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,what,kw", HC.REFUSALS, ids=[f"{e}-{w}".replace(" ", "_") for e, w, _ in HC.REFUSALS])
def test_bad_arguments_are_refused_before_any_launch(entry, what, kw):
    lib, nat, F = _lib()
    p = F._p
    kw = dict(kw)
    B, P, D, K, G = kw.get("B", 1), kw.get("P", 2), kw.get("D", 512), kw.get("K", 4), kw.get("G", 2)
    mode, has_pw = HC.POOL_CODE[kw.get("mode", "mean")], kw.get("pool_w", True)
    n = (B + 1) * (G + 1) * 17 * 1040 + 4096                    # more floats than any argument of these calls addresses
    f = lambda: torch.full((n,), SENT, dtype=torch.float32, device=_dev())  # noqa: E731
    ins = [torch.ones(n, dtype=torch.float32, device=_dev()) for _ in range(8)]
    outs = [f() for _ in range(9)]
    ws = torch.zeros(max(n, lib.vlsa_head_workspace_bytes(512)), dtype=torch.float32, device=_dev())
    pw = p(ins[1]) if has_pw else None
    s = F._stream()
    o = [p(t) for t in outs]
    if entry == "head_forward":
        rc = lib.vlsa_head_forward(p(ins[0]), P, D, mode, pw, p(ins[2]), p(ins[3]), p(ins[4]), K, p(ins[5]), p(ws), *o[:6], s)
    elif entry == "head_batch":
        rc = lib.vlsa_head_forward_batch(p(ins[0]), B, P, D, mode, pw, p(ins[2]), p(ins[3]), p(ins[4]), K, p(ins[5]), p(ws), *o[:6], s)
    elif entry == "head_batch_text":
        pooled = p(ins[0]) if kw.get("layout") == "inplace" else o[2]
        rc = lib.vlsa_head_forward_batch_text(p(ins[0]), B, P, D, mode, pw, p(ins[2]), p(ins[3]), p(ins[4]), K, p(ins[5]), o[0], o[1], pooled,
                                              *o[3:8], s)
    elif entry == "merge_head":
        rc = lib.vlsa_vlfan_merge_head(p(ins[0]), p(ins[6]), p(ins[7]), G, P, D, mode, pw, p(ins[2]), p(ins[3]), p(ins[4]), K, p(ins[5]), p(ws),
                                       *o[:9], s)
    elif entry == "merge_head_batch":
        st = [16, 16, P * D, 16 * G, 16 * G, G * P * D, 16, 16, P * D]
        if not kw.get("strides_ok", True):
            st[2] += 2                                          # the partial stride of pacc: no multiple of 4
        rc = lib.vlsa_vlfan_merge_head_batch_strided(p(ins[0]), p(ins[6]), p(ins[7]), B, G, P, D, (ctypes.c_int64 * 9)(*st), mode, pw, p(ins[2]),
                                                     p(ins[3]), p(ins[4]), K, p(ins[5]), *o[:9], s)
    elif entry == "head_backward":
        rc = lib.vlsa_head_backward_batch(p(ins[0]), None, None, p(ins[1]), p(ins[2]), p(ins[3]), p(ins[4]), p(ins[5]), p(ins[6]), p(ins[7]),
                                          p(ins[5]), B, P, D, K, o[0], *o[1:6], s)
    else:
        rc = lib.vlsa_query_chain(p(ins[0]), p(ins[1]), kw.get("nq", 3), int(kw.get("gated", False)), D, o[0], s)
    torch.cuda.synchronize()
    assert rc == nat.EINVAL, (entry, what, rc)
    assert all(bool((t == SENT).all()) for t in outs) and float(ws.abs().max()) == 0.0, "a refused call wrote something"


@pytest.mark.parametrize("which", ["sa", "ba", "oo"])
def test_every_strided_merge_stride_is_checked(which):
    lib, nat, F = _lib()
    p = F._p
    st = [16, 16, 2 * 512, 32, 32, 2 * 2 * 512, 16, 16, 2 * 512]
    st[{"sa": 2, "ba": 5, "oo": 8}[which]] += 2
    t = [torch.full((40_000,), SENT, dtype=torch.float32, device=_dev()) for _ in range(16)]
    rc = lib.vlsa_vlfan_merge_head_batch_strided(p(t[0]), p(t[1]), p(t[2]), 3, 2, 2, 512, (ctypes.c_int64 * 9)(*st), 0, None, p(t[3]), p(t[4]),
                                                 p(t[5]), 4, p(t[6]), *(p(x) for x in t[7:16]), F._stream())
    torch.cuda.synchronize()
    assert rc == nat.EINVAL and all(bool((x == SENT).all()) for x in t[7:])


# ---- module level: head_forward('given') and head_train(P = 1) behind VLSA.forward / _deepmil_logits ----------------------------------------
def _vlsa_deepmil(width, K=4):
    from vlsa_amd.vlsa import VLSA
    cfg = dict(name="DeepMIL", dim_in=512, dim_hid=256, num_cls=width, use_feat_proj=False, drop_rate=0.0, pooling="gated_attention",
               pred_head="default")
    torch.manual_seed(11 + width)
    return VLSA.from_modules(cfg, pretrained_text_features=torch.randn(K, width) * 2, logit_scale_init=HC.LOGIT_SCALE).to(_dev())


def _fallback64(net, feats):
    """the torch-ops fallback of VLSA.forward (both F.normalize calls, exp(logit_scale) * v^ T^^T) in float64, differentiable"""
    T = net._text_features().double()
    Th = T / T.norm(dim=-1, keepdim=True).clamp_min(HC.NORM_EPS)
    v = feats.double()
    vh = v / v.norm(dim=-1, keepdim=True).clamp_min(HC.NORM_EPS)
    return net.logit_scale.double().exp() * vh @ Th.t(), vh, Th


def _bag(n, seed):
    import cases
    return cases.make_bag(n, seed, "clustered").to(_dev())


@pytest.mark.parametrize("width", [256, 768])
def test_vlsa_forward_of_a_deepmil_encoder_without_gradient(width, monkeypatch):
    from vlsa_amd import functional as VF
    net = _vlsa_deepmil(width).eval()
    X = _bag(333, 40 + width)[None]
    calls = []
    real = VF.head_forward
    monkeypatch.setattr(VF, "head_forward", lambda rows, pool, *a, **k: calls.append((pool, tuple(rows.shape))) or real(rows, pool, *a, **k))
    with torch.no_grad():
        logits, vhat, That = net(X)
        rl, rv, rt = _fallback64(net, net.encode_instances(X))
    assert calls == [("given", (1, width))], calls        # the head kernel ran, not the torch-ops fallback
    for name, got, ref, g in (("logits", logits, rl, HC.GATE_LOGITS), ("vhat", vhat, rv, HC.GATE_VHAT), ("That", That, rt, HC.GATE_THAT)):
        e = HC.err_of(got.cpu(), ref.cpu())
        print(f"[head paths] VLSA.forward no-grad width {width} {name}: {e:.3e} (gate {g:.1e})")
        assert got.shape == ref.shape and e <= g, name


def _grads_of(net, outs, G):
    net.zero_grad(set_to_none=True)
    logits, vhat = outs[0], outs[1]
    ((logits.double() * G[0]).sum() + (vhat.double() * G[1]).sum()).backward()
    return {n: p.grad.detach().double().cpu().clone() for n, p in net.named_parameters() if p.grad is not None}


def _check_train(net, got, ref, what):
    gen = torch.Generator().manual_seed(5)
    G = [torch.randn(ref[0].shape, generator=gen).double().to(_dev()), torch.randn(ref[1].shape, generator=gen).double().to(_dev())]
    for name, a, b, g in (("logits", got[0], ref[0], HC.GATE_LOGITS), ("vhat", got[1], ref[1], HC.GATE_VHAT), ("That", got[2], ref[2], HC.GATE_THAT)):
        e = HC.err_of(a.detach().cpu(), b.detach().cpu())
        print(f"[head paths] {what} {name}: {e:.3e} (gate {g:.1e})")
        assert a.shape == b.shape and e <= g, name
    g_ref, g_got = _grads_of(net, ref, G), _grads_of(net, got, G)
    assert set(g_ref) == set(g_got) and "logit_scale" in g_ref
    big = max(float(t.abs().max()) for t in g_ref.values())
    for n in g_ref:
        # the score layer's output bias: its gradient is the sum of dL/da over a bag, exactly zero under a softmax pooling, so both routes
        # return rounding noise there -- measured against the module's largest gradient (the rule of test_gpu_deepmil_train_batch.py)
        is_c = n.endswith("sigma.fc2.bias") or n.endswith("sigma.attention.2.bias")
        g = HC.GATE_GRAD * (big if is_c else float(g_ref[n].abs().max()))
        e = HC.err_of(g_got[n], g_ref[n])
        print(f"[head paths] {what} d {n}: {e:.3e} (gate {g:.1e})")
        assert e <= g, n


@pytest.mark.parametrize("width", [256, 768])
def test_vlsa_forward_of_a_deepmil_encoder_with_gradient(width):
    """head_train with B = P = 1 behind VLSA.forward: outputs and every parameter gradient against the fallback in float64 on the same
    encoder output (the encoder's own backward runs in both, so a difference is the head's)"""
    net = _vlsa_deepmil(width).train()
    X = _bag(333, 50 + width)[None]
    got = net(X)
    assert got[0].grad_fn is not None and "HeadTrain" in type(got[0].grad_fn).__name__
    _check_train(net, got, _fallback64(net, net.encode_instances(X)), f"VLSA.forward grad width {width}")


@pytest.mark.parametrize("width", [256, 768])
def test_deepmil_logits_of_nine_bags(width):
    net = _vlsa_deepmil(width).train()
    feats = torch.cat([net.encode_instances(_bag(100 + 37 * i, 60 + i)[None]) for i in range(9)])
    got = net._deepmil_logits(feats, net._text_features())
    assert "HeadTrain" in type(got[0].grad_fn).__name__
    feats2 = torch.cat([net.encode_instances(_bag(100 + 37 * i, 60 + i)[None]) for i in range(9)])
    _check_train(net, got, _fallback64(net, feats2), f"_deepmil_logits 9 bags width {width}")
