"""DeepAttnMISL, the parts that need no GPU: the float64 helper against every fixture, its empty-cluster and out-of-range rules, the
state-dict keys against the reference's list in the fixtures, the refusals that need no device, the factory's standing refusal, the
``patch_reference_deepattnmisl`` round trip and the C ABI's host-side checks."""
import ctypes
import glob
import os
import sys
import types

import numpy as np
import pytest
import torch

import deepattnmisl_cases as AC
import deepattnmisl_helpers as AH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(AC.CASES))
def test_helper_reproduces_the_fixture(name):
    N, Kc, num_cls, rows, seed = AC.CASES[name]
    x, ids, params, w = AC.make_case(name)
    fx = AH.load_fixture(name)
    logits, hc, pre, grads = AH.run64(x, ids, [torch.from_numpy(params[k]) for k in AC.KEYS], Kc, w)
    assert np.abs(logits - fx["logits"]).max() <= 1e-10 and np.abs(hc - fx["hc"]).max() <= 1e-10
    for k in AC.KEYS:         # float64 entries to 1e-10; the four tensors stored as float32 to that rounding (6e-8 of an entry)
        tol = 1e-10 if k not in AC.ROUNDED else 1e-7 * float(fx["gmax/" + k]) + 1e-10
        assert np.abs(grads[k] - fx["grad/" + k]).max() <= tol, k
    r, u = np.nonzero(np.abs(pre) < AC.NEAR_ZERO)
    assert r.tolist() == fx["near_row"].tolist() and u.tolist() == fx["near_unit"].tolist()
    assert np.abs(pre[r, u] - fx["near_value"]).max() <= 1e-10 if len(r) else True
    assert int(fx["ref32_mask_flips"]) == 0 and int(np.bincount(ids, minlength=Kc).min()) >= 1


def test_fixture_files_are_the_cases_and_stay_under_the_size_limit():
    gold = os.path.join(ROOT, "tests", "golden")
    files = sorted(glob.glob(os.path.join(gold, "deepattnmisl_*.npz")))
    assert files == sorted(os.path.join(gold, f"deepattnmisl_{n}{t}.npz") for n in AC.CASES for t in ("", "_gp"))
    assert max(os.path.getsize(f) for f in files) < 1 << 20


def test_helper_empty_cluster_is_a_zero_row_and_out_of_range_ids_join_no_cluster():
    x, _, params, w = AC.make_case("n17")
    P = [torch.from_numpy(params[k]) for k in AC.KEYS]
    ids = np.array([0, 0, 1, 1, 4, 4, 5, 5, 7, 7, -1, 8, 100, 0, 1, 4, 5])          # clusters 2, 3, 6 empty; rows 10-12 in none
    _, hc, pre, grads = AH.run64(x, ids, P, 8, w)
    assert np.all(hc[[2, 3, 6]] == 0) and np.all(np.isfinite(grads["phis.0.weight"]))
    keep = (ids >= 0) & (ids < 8)
    _, hc2, _, _ = AH.run64(x[keep], ids[keep], P, 8, w)
    assert np.abs(hc - hc2).max() <= 1e-12
    h = np.maximum(pre, 0)
    assert np.abs(hc[4] - h[[4, 5, 15]].mean(axis=0)).max() <= 1e-12
    _, hc3, _, _ = AH.run64(x, ids, P, 8, w, mask=torch.zeros(17, 256, dtype=torch.bool))       # a given mask is taken
    assert np.all(hc3 == 0)


def test_state_dict_keys_and_shapes_equal_the_reference_list():
    from vlsa_amd import DeepAttnMISL
    from vlsa_amd.deepmil import DeepAttnMISL as direct
    assert DeepAttnMISL is direct
    for name, (N, Kc, num_cls, rows, seed) in AC.CASES.items():
        fx = AH.load_fixture(name)
        sd = DeepAttnMISL(dim_in=512, dim_hid=256, num_cls=num_cls, num_clusters=Kc).state_dict()
        assert list(sd) == list(fx["keys"]) == list(AC.KEYS)
        for k in AC.KEYS:
            assert tuple(sd[k].shape) == tuple(fx["shape/" + k]) == AC.shapes(Kc, num_cls)[k], k


def test_cpu_bag_and_uncovered_shapes_raise():
    from vlsa_amd import DeepAttnMISL, VlsaNativeError
    ids = torch.zeros(10)
    with pytest.raises(VlsaNativeError):
        DeepAttnMISL().eval()(torch.randn(1, 10, 512), ids)
    with pytest.raises(VlsaNativeError):
        DeepAttnMISL(dim_in=1024).eval()(torch.randn(1, 10, 1024), ids)
    with pytest.raises(VlsaNativeError):
        DeepAttnMISL(num_clusters=17).eval()(torch.randn(1, 10, 512), ids)


def test_the_factory_still_refuses_deepattnmisl():
    from vlsa_amd.model_utils import load_model
    with pytest.raises(NotImplementedError, match="cluster"):
        load_model("DeepMIL", [512, 256, 1], network="DeepAttnMISL")


def test_patch_round_trip_on_stand_in_modules(monkeypatch):
    from vlsa_amd.deepmil import DeepAttnMISL
    from vlsa_amd.model_utils import patch_reference_deepattnmisl, unpatch_reference_deepattnmisl
    mods = {}
    for full in ("model", "model.deepmil", "model.utils", "runner", "runner.sa_handler"):
        mods[full] = types.ModuleType(full)
        monkeypatch.setitem(sys.modules, full, mods[full])
        if "." in full:
            setattr(mods[full.split(".")[0]], full.split(".")[1], mods[full])
    original = type("Original", (), {})
    mods["model.deepmil"].DeepAttnMISL = mods["runner.sa_handler"].DeepAttnMISL = original       # model.utils has none: absent before
    saved = patch_reference_deepattnmisl()
    assert all(mods[m].DeepAttnMISL is DeepAttnMISL for m in ("model.deepmil", "model.utils", "runner.sa_handler"))
    unpatch_reference_deepattnmisl(saved)
    assert mods["model.deepmil"].DeepAttnMISL is original and mods["runner.sa_handler"].DeepAttnMISL is original
    assert not hasattr(mods["model.utils"], "DeepAttnMISL")


@pytest.mark.skipif(not os.path.isdir("/root/reference/model"), reason="needs the upstream reference at /root/reference")
def test_patch_round_trip_on_the_reference_and_its_factory_builds_ours():
    from _ref_import import import_reference
    from vlsa_amd.deepmil import DeepAttnMISL
    from vlsa_amd.model_utils import patch_reference_deepattnmisl, unpatch_reference_deepattnmisl
    import_reference()
    import model.deepmil as ref_mil
    import model.utils as ref_utils
    before = (ref_mil.DeepAttnMISL, ref_utils.DeepAttnMISL)
    saved = patch_reference_deepattnmisl()
    try:
        assert ref_mil.DeepAttnMISL is DeepAttnMISL and ref_utils.DeepAttnMISL is DeepAttnMISL
        built = ref_utils.load_model("DeepMIL", [512, 256, 1], network="DeepAttnMISL", num_clusters=8)
    finally:
        unpatch_reference_deepattnmisl(saved)
    assert (ref_mil.DeepAttnMISL, ref_utils.DeepAttnMISL) == before and type(built) is DeepAttnMISL


@pytest.fixture(scope="module")
def lib():
    from vlsa_amd import build, _native
    build.build_native()
    return _native.load()


def test_parts_and_workspace_sizes_depend_on_the_row_count_alone(lib):
    tile = lib.vlsa_cluster_pool_tile_rows()
    assert tile == 64 and lib.vlsa_cluster_pool_backward_tile_rows() == 32
    assert [lib.vlsa_cluster_pool_parts(n) for n in (0, 1, tile, tile + 1, 2798, 50000, 10 ** 7)] == [1, 1, 1, 2, 44, 128, 128]
    assert lib.vlsa_cluster_pool_workspace_bytes(44, 8) == 16 * 16 * 3 * 1024 + 44 * (8 * 256 + 16) * 4
    assert lib.vlsa_cluster_pool_workspace_bytes(0, 8) == 0 and lib.vlsa_cluster_pool_workspace_bytes(4, 17) == 0
    per = (256 * 512 + 256) * 4
    assert [lib.vlsa_cluster_pool_backward_workspace_bytes(n) for n in (0, 1, 4, 5, 88, 10 ** 6)] == [0, per, per, 2 * per, 22 * per, 64 * per]
    assert 64 * per <= 32.2 * 2 ** 20          # the bound the header states


P = ctypes.c_void_p(0x1000)      # any non-null address: every call below must be refused before anything is dereferenced or launched


def _fwd(lib, B=2, D=512, H=256, Kc=8, desc=P, ps=P, n=4, off=P, ids=P, Wp=P, ws=P, hc=P, cnt=P, dt=1):
    return lib.vlsa_cluster_pool_forward_batch(desc, B, dt, D, H, Kc, ps, n, off, ids, Wp, P, ws, hc, cnt, None, None)


def _bwd(lib, B=2, D=512, H=256, Kc=8, desc=P, ps=P, n=4, off=P, ids=P, mask=P, ws=P, dhc=P, cnt=P, dt=1):
    return lib.vlsa_cluster_pool_backward_batch(desc, B, dt, D, H, Kc, ps, n, off, ids, mask, dhc, cnt, ws, P, P, None)


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_bad_arguments_are_refused_on_the_host(lib, call):
    for kw in ({"B": 0}, {"B": 65}, {"desc": None}, {"ps": None}, {"n": 1}, {"Kc": 0}, {"off": None}, {"ids": None}, {"ws": None}, {"cnt": None}):
        assert call(lib, **kw) == -1, (call.__name__, kw)
    for kw in ({"D": 256}, {"D": 1024}, {"H": 128}, {"Kc": 17}, {"dt": 7}):
        assert call(lib, **kw) == -2, (call.__name__, kw)
    assert _fwd(lib, Wp=None) == -1 and _fwd(lib, hc=None) == -1 and _bwd(lib, mask=None) == -1 and _bwd(lib, dhc=None) == -1


def test_the_part_table_formula_is_the_library_function(lib):
    """the one torch expression that fills every route's part_start on the device (``part_counts``, called by ``_ChunkPlan.part_table``
    with the rows and the cap asked of the library) against the library's own *_parts(n), around every boundary of rows and cap"""
    from vlsa_amd.functional import part_counts
    routes = {"dsmil": (lib.vlsa_dsmil_part_rows, lib.vlsa_dsmil_parts), "cluster_pool": (lib.vlsa_cluster_pool_tile_rows, lib.vlsa_cluster_pool_parts),
              "ilra": (lib.vlsa_ilra_pool_part_rows, lib.vlsa_ilra_pool_parts)}
    for name, (rows_of, parts_of) in routes.items():
        rows, cap = rows_of(), parts_of(1 << 62)
        ns = [1, 2, rows - 1, rows, rows + 1, 2798, rows * cap - 1, rows * cap, rows * cap + 1, 20000, 50000, 10 ** 7, 2 ** 40]
        want = [parts_of(n) for n in ns]
        assert part_counts(torch.tensor(ns, dtype=torch.int64), rows, cap).tolist() == want, name
        assert want[3:5] == [1, 2] and want[7:9] == [cap, cap] and want[6] == cap and want[-1] == cap, name
    assert {k: (r(), p(1 << 62)) for k, (r, p) in routes.items()} == {"dsmil": (512, 64), "cluster_pool": (64, 128), "ilra": (256, 64)}


def test_ids_that_match_no_cluster_become_minus_one_before_the_cast():
    from vlsa_amd.functional import cluster_ids_int32
    inf, nan = float("inf"), float("nan")
    f = torch.tensor([[0.0, 7.0, 8.0, -1.0, 2.5, 1e10, 2.0 ** 32 + 3, inf, -inf, nan, 3.0]])          # [1, N] floats, as the loader's
    i = torch.tensor([0, 7, 8, -1, 2 ** 32 + 3, -2 ** 31, 2 ** 62, 5], dtype=torch.int64)
    out = cluster_ids_int32([f, i], [11, 8], "cpu", 8)
    assert out.dtype == torch.int32 and out.tolist() == [0, 7, -1, -1, -1, -1, -1, -1, -1, -1, 3] + [0, 7, -1, -1, -1, -1, -1, 5]
    with pytest.raises(ValueError):
        cluster_ids_int32([f], [12], "cpu", 8)
