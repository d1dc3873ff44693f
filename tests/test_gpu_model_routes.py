"""Which HIP kernels every batched model route launches, pinned: the encoders' ``forward_bags`` / ``pool_bags`` / ``aggregate_bags`` /
``cluster_features`` decide in Python which launch chain a list of bags takes (batched or bag by bag, HIP or torch, one autograd node or
many), and nothing else in the suite notices when an input changes its chain while the numbers stay right.  For every case of
``CASES`` and every input of ``INPUTS`` the kernels of ONE call on fresh bag collections (torch profiler, device activity, names with
counts; the runtime's host-side calls and the copy engine's copies and fills are not kernels) must equal
``model_routes_expected.json``, and a second, identically seeded model must return the same bits.  A case runs once per dtype, each
time with fresh models: the first input of a run is the one that packs the weights.

The recording is data: ``python tests/test_gpu_model_routes.py OUT.json`` writes it.  A case whose list differs from it has changed
its route: that is to be fixed in the code, not in the recording.  (A change that means to move a route records afresh and says which
cases moved and why.)"""
import contextlib
import functools
import io
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "model_routes_expected.json")
ROWS = (17, 65)                    # on each side of the kernels' 64-row tiles
COUNTS = (1, 3, 64, 65)            # 65: the smallest count that takes two chunks
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
INPUTS = [(n, kind) for n in COUNTS for kind in ("list", "set")]
K = 4                              # classes of the text side

_BAGS = {}


def _bags(dtype_name, n):
    """the first n of 65 resident bags of 17 / 65 rows in turn (made once per dtype, never written)"""
    if dtype_name not in _BAGS:
        g = torch.Generator().manual_seed(1234)
        _BAGS[dtype_name] = [torch.randn(ROWS[i % 2], 512, generator=g).to(DTYPES[dtype_name]).cuda() for i in range(max(COUNTS))]
    return _BAGS[dtype_name][:n]


def _collection(dtype_name, n, kind):
    from vlsa_amd import functional as VF
    bags = list(_bags(dtype_name, n))
    return VF.BagSet(bags) if kind == "set" else bags          # a fresh set: none of its tables is up, none of its plans built


# ---- the models ---------------------------------------------------------------------------------------------------------------------
def _vlsa(cfg):
    from vlsa_amd.vlsa import VLSA
    T = torch.randn(K, 512, generator=torch.Generator().manual_seed(77))
    return VLSA.from_modules(cfg, pretrained_text_features=T, logit_scale_init=4.0).cuda().eval()


def _deepmil(pooling, proj, head, train=False, rates=None):
    """proj: None | 'frozen' | 'trains'; rates: the gated module's two dropout rates set by hand"""
    cfg = dict(name="DeepMIL", dim_in=512, dim_hid=256, num_cls=512, use_feat_proj=proj is not None, drop_rate=0.25, pooling=pooling,
               pred_head=head, dim_reduction=4, keep_ratio=0.8)
    m = _vlsa(cfg)
    if proj == "frozen":
        m.mil_encoder.feat_proj.requires_grad_(False)
    if rates is not None:
        m.mil_encoder.sigma.fc1[2].p, m.mil_encoder.sigma.score[2].p = rates
    return m.train(train)


def _featmil(pooling):
    return _vlsa(dict(name="FeatMIL", dim_in=512, pooling=pooling))


def _vlfan(proj):
    from vlsa_amd.deepmil import VLFAN
    return VLFAN(dim_in=512, dim_hid=256, use_feat_proj=proj, drop_rate=0.0, query="Parameter", num_query=6, query_pooling="mean").cuda().eval()


def _dsmil(proj, train=False):
    from vlsa_amd.deepmil import DSMIL
    m = DSMIL(dim_in=512, dim_hid=256, num_cls=4, use_feat_proj=proj, drop_rate=0.25).cuda()
    if proj:
        m.feat_proj.requires_grad_(False)
    return m.train(train)


def _deepattnmisl():
    from vlsa_amd.deepmil import DeepAttnMISL
    return DeepAttnMISL(dim_in=512, dim_hid=256, num_cls=4, num_clusters=8).cuda().eval()


def _ilra():
    from vlsa_amd.deepmil import ILRA
    with contextlib.redirect_stdout(io.StringIO()):
        m = ILRA(dim_in=512, dim_hid=256, num_cls=4, num_layers=2).cuda().eval()
    m.ROW_BUDGET = 100             # 17 + 65 + 17 rows fill a chunk: the budget closes chunks at these sizes, before the 64-bag cap does
    return m


# ---- the calls ----------------------------------------------------------------------------------------------------------------------
def _backward(out):
    first = out[0] if isinstance(out, (tuple, list)) else out
    first.float().sum().backward()
    return out


def _enc_grad(m, bags, **kw):                    # DeepMIL.forward_bags with its graph, and the backward behind it
    return _backward(m.mil_encoder.forward_bags(bags, **kw))


def _net_nograd(m, bags):                        # VLSA.forward_bags without a gradient: DeepMIL.pool_bags / the FeatMIL branch
    with torch.no_grad():
        return m.forward_bags(bags)


def _grad(fn):
    return lambda m, bags: _backward(getattr(m, fn)(bags))


def _cluster(m, bags):
    ids = [torch.arange(x.shape[0], dtype=torch.float32) % 8 for x in bags]       # CPU floats, as the reference's loader hands them
    return _backward(m.forward_bags(bags, ids))


def _ilra_forward(m, bags):                      # the chunking is the forward's: 22 chunks with a float64 tail each, no backward behind them
    return m.forward_bags(bags)


def _cases():
    c = {}
    for pooling in ("mean", "max", "attention", "gated_attention"):
        for proj in (None, "frozen", "trains"):
            for head in ("default", "Adapter"):
                for train in ((False, True) if pooling == "gated_attention" else (False,)):
                    tag = f"deepmil-{pooling}-proj_{proj}-{head}-{'train' if train else 'eval'}"
                    build = (lambda pooling=pooling, proj=proj, head=head, train=train: _deepmil(pooling, proj, head, train))
                    c[tag + "-enc_grad"] = (build, _enc_grad)
                    c[tag + "-net_nograd"] = (build, _net_nograd)
    for train in (False, True):                   # unequal rates: the input on which the sites' conditions differ
        tag = f"deepmil-gated_attention-rates_unequal-{'train' if train else 'eval'}"
        build = (lambda train=train: _deepmil("gated_attention", None, "default", train, rates=(0.25, 0.5)))
        c[tag + "-enc_grad"] = (build, _enc_grad)
        c[tag + "-net_nograd"] = (build, _net_nograd)
    for pooling in ("attention", "gated_attention"):
        c[f"deepmil-{pooling}-with_attn-enc_grad"] = ((lambda pooling=pooling: _deepmil(pooling, None, "default")),
                                                      lambda m, bags: _enc_grad(m, bags, ret_with_attn=True))
    for pooling in ("mean", "max", "logit_top3"):
        c[f"featmil-{pooling}-net_nograd"] = ((lambda pooling=pooling: _featmil(pooling)), _net_nograd)
    for proj in (False, True):
        c[f"vlfan-proj_{proj}-forward_bags"] = ((lambda proj=proj: _vlfan(proj)), _grad("forward_bags"))
        c[f"vlfan-proj_{proj}-aggregate_bags"] = ((lambda proj=proj: _vlfan(proj)), _grad("aggregate_bags"))
    c["dsmil-proj_none-eval"] = (lambda: _dsmil(False), _grad("forward_bags"))
    c["dsmil-proj_frozen-eval"] = (lambda: _dsmil(True), _grad("forward_bags"))
    c["dsmil-proj_none-train"] = (lambda: _dsmil(False, True), _grad("forward_bags"))
    c["deepattnmisl"] = (_deepattnmisl, _cluster)
    c["ilra-row_budget_100"] = (_ilra, _ilra_forward)
    return c


CASES = _cases()


# ---- recording and comparing ----------------------------------------------------------------------------------------------------------
def _kernels(fn):
    """(what fn returned, {kernel name: launches}) -- the torch profiler's device activity without the runtime's own calls (hipLaunchKernel,
    hipMemcpyAsync, hipMalloc ...: they depend on the allocator's state) and without the copy engine's entries"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = {}
    for e in prof.key_averages():
        if not e.key.lower().startswith(("hip", "memcpy", "memset")):
            names[e.key] = names.get(e.key, 0) + e.count
    return out, names


def _leaves(out):
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in _leaves(o)]
    assert out is None or isinstance(out, dict), type(out)
    return [] if out is None else [t for k in sorted(out) for t in _leaves(out[k])]


def _twin(build):
    torch.manual_seed(5)
    return build()


def run_case(name, d):
    """{input id: {kernel name: launches}} of one case on bags of dtype d; asserts that a twin model gives the same bits on every input"""
    build, call = CASES[name]
    call(_twin(build), _collection(d, 1, "list"))          # whatever the libraries under this route do once per process: not a launch of a case
    a, b = _twin(build), _twin(build)
    got = {}
    for n, kind in INPUTS:
        outs = []
        for m in (a, b):
            m.zero_grad(set_to_none=True)
            torch.manual_seed(9)
            bags = _collection(d, n, kind)
            if m is a:
                out, got[f"{n}-{kind}"] = _kernels(lambda: call(m, bags))
            else:
                out = call(m, bags)
            outs.append([t.detach() for t in _leaves(out)])
        assert len(outs[0]) == len(outs[1]) > 0
        for x, y in zip(*outs):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), (name, d, n, kind)
    return got


@functools.lru_cache(maxsize=None)
def _load():
    with open(EXPECTED) as f:
        rec = json.load(f)
    lists = [{rec["names"][i]: k for i, k in lst} for lst in rec["lists"]]
    return {case: {inp: lists[j] for inp, j in per.items()} for case, per in rec["cases"].items()}


@pytest.mark.parametrize("d", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_route_launches_the_recorded_kernels(name, d):
    want = _load()[f"{name}/{d}"]
    got = run_case(name, d)
    assert sorted(got) == sorted(want)
    for inp in got:
        if got[inp] != want[inp]:
            diff = {k: (want[inp].get(k, 0), got[inp].get(k, 0)) for k in set(want[inp]) | set(got[inp]) if want[inp].get(k, 0) != got[inp].get(k, 0)}
            raise AssertionError(f"{name} / {d}-{inp}: launches changed, kernel: (recorded, now) = {diff}")


def record(path):
    import time
    names, lists, cases = {}, {}, {}
    for name in [f"{c}/{d}" for c in sorted(CASES) for d in sorted(DTYPES)]:
        t0 = time.perf_counter()
        per = {}
        for inp, ks in run_case(*name.split("/")).items():
            key = tuple(sorted((names.setdefault(k, len(names)), n) for k, n in ks.items()))
            per[inp] = lists.setdefault(key, len(lists))
        cases[name] = per
        print(f"{name}: {time.perf_counter() - t0:.2f} s, {len(set(per.values()))} distinct lists", flush=True)
    with open(path, "w") as f:
        # one line per kernel name, per list and per case: a change of the recording shows as the lines it touches
        rows = lambda xs: ",\n".join(json.dumps(x, separators=(",", ":")) for x in xs)  # noqa: E731
        f.write('{"names": [\n' + rows(names) + '\n],\n"lists": [\n' + rows([list(p) for p in key] for key in lists) + '\n],\n"cases": {\n'
                + ",\n".join(json.dumps(k) + ": " + json.dumps(cases[k], separators=(",", ":"), sort_keys=True) for k in sorted(cases)) + "\n}}\n")
    print(f"{len(cases)} cases, {len(lists)} distinct lists, {len(names)} kernel names -> {path}")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    record(sys.argv[1])
