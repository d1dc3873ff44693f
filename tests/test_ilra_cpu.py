"""ILRA, the parts that need no GPU: the float64 restatement against every fixture of the reference's float64 run (logits and
intermediates to 1e-9, gradient digests to 1e-8 of the tensor's scale), the fixtures' own gates, keys / shapes / initialisation against
the reference's list, the refusals that need no device, the factory's standing refusal, the ``patch_reference_ilra`` round trip and the
C ABI's host-side checks."""
import contextlib
import ctypes
import glob
import io
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

import ilra_cases as IC
import ilra_helpers as IH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(IC.CASES))
def test_restatement_reproduces_the_fixture(name):
    N, rows, num_layers, num_cls, seed, recipe = IC.CASES[name]
    x, params, w = IC.make_case(name)
    fx = IH.load_fixture(name)
    logits, inter, grads = IH.run64(x, params, num_layers, w)
    assert list(fx["keys"]) == list(params) == list(grads)
    el = float(np.abs(logits - fx["logits"]).max())
    assert el <= 1e-9 * max(1.0, float(np.abs(fx["logits"]).max())), (name, el)
    for i in range(num_layers):
        for k in (f"Z{i}", f"H{i}"):
            assert np.abs(inter[k] - fx[k]).max() <= 1e-9 * max(1.0, float(np.abs(fx[k]).max())), (name, k)
        assert abs(float(np.abs(inter[f"xhat{i}"]).max()) - float(fx[f"xmax{i}"])) <= 1e-9 * float(fx[f"xmax{i}"]), (name, i)
    assert np.abs(inter["Zp"] - fx["Zp"]).max() <= 1e-9 * max(1.0, float(np.abs(fx["Zp"]).max())), name
    IH.check_digests(name, grads, fx, seed, 1e-8)
    assert abs(min(float(np.abs(t).min()) for t in inter["tail_pre"]) - float(fx["relu/min_abs_tail"])) <= 1e-9
    assert abs(min(float(np.abs(inter[f"t{i}"]).min()) for i in range(num_layers)) - float(fx["relu/min_abs_rows"])) <= 1e-9


@pytest.mark.parametrize("name", IC.PARITY)
def test_fixture_gates_hold(name):
    """what the generator asserted: the case is alive (a dropped row shows), the reference's own fp32 run is close, no tail ReLU sits at
    zero; and the mask band covers every decision the reference's fp32 run flips"""
    N = IC.CASES[name][0]
    fx = IH.load_fixture(name)
    assert float(fx["referr/logits"]) <= 1e-5 * float(np.abs(fx["logits"]).max())
    assert N == 1 or float(fx["sens/drop_last"]) >= 1e-3
    assert float(fx["relu/min_abs_tail"]) >= 1e-4
    assert IC.BAND >= 1e-6 and IC.BAND >= 10 * float(fx["relu/ref32_flip_max"])


def test_zero_gradients_of_the_one_key_attention_are_exact():
    """project_backward has one key: fc_k and the q / k thirds of its in_proj get exact zeros"""
    x, params, w = IC.make_case("n17")
    _, _, grads = IH.run64(x, params, 2, w)
    for i in range(2):
        pb = f"gab_blocks.{i}.project_backward."
        assert not grads[pb + "fc_k.weight"].any() and not grads[pb + "fc_k.bias"].any()
        assert not grads[pb + "multihead_attn.in_proj_weight"][:512].any() and grads[pb + "multihead_attn.in_proj_weight"][512:].any()
        assert not grads[pb + "multihead_attn.in_proj_bias"][:512].any()


def test_given_masks_are_taken():
    x, params, w = IC.make_case("n17")
    l0, inter, _ = IH.run64(x, params, 2, w)
    same, _, _ = IH.run64(x, params, 2, w, masks=[inter["t0"] > 0, inter["t1"] > 0])
    other, _, _ = IH.run64(x, params, 2, w, masks=[np.zeros((17, 256), bool)] * 2)
    assert np.array_equal(l0, same) and np.abs(other - l0).max() > 1e-3


def test_fixture_files_are_the_cases_and_stay_under_the_size_limit():
    gold = os.path.join(ROOT, "tests", "golden")
    files = sorted(glob.glob(os.path.join(gold, "ilra_*.npz")))
    assert files == sorted(os.path.join(gold, f"ilra_{n}.npz") for n in IC.CASES)
    assert max(os.path.getsize(f) for f in files) < 1 << 20


def _quiet(**kw):
    from vlsa_amd import ILRA
    with contextlib.redirect_stdout(io.StringIO()):
        return ILRA(**kw)


def test_keys_shapes_and_initialisation_equal_the_reference_list(capsys):
    from vlsa_amd import ILRA
    from vlsa_amd.deepmil import ILRA as direct
    assert ILRA is direct
    with open(os.path.join(ROOT, "tests", "golden", "ilra_keys.json")) as f:
        ref = json.load(f)
    for tag, want in ref.items():
        L, C = (int(v) for v in tag.split("/"))
        torch.manual_seed(5)
        m = ILRA(dim_in=512, dim_hid=256, num_cls=C, num_layers=L)
        assert "[setup] initialized an ILRA model." in capsys.readouterr().out
        sd = m.state_dict()
        assert list(sd) == [k for k, _ in want] == list(IC.shapes(L, C))
        assert all(list(sd[k].shape) == sh for k, sh in want)
        for k, v in sd.items():          # the reference's initial distributions (initialize_weights, nn.MultiheadAttention, xavier_uniform_)
            if k.endswith("latent") or k.endswith(".S"):
                assert float(v.abs().max()) <= np.sqrt(6 / 512) and float(v.std()) > 0.04
            elif k.endswith("in_proj_weight"):
                assert float(v.abs().max()) <= np.sqrt(6 / 1024) and abs(float(v.std()) - np.sqrt(2 / 1024)) < 2e-3
            elif k.endswith("weight") and v.shape[0] >= 256:
                assert abs(float(v.std()) - np.sqrt(2.0 / (v.shape[0] + v.shape[1]))) < 2e-3 and float(v.abs().max()) > 3 * float(v.std())
            elif k.endswith("in_proj_bias") or k.endswith("out_proj.bias"):
                assert not v.any()
    ln = _quiet(ln=True, topk=2, dim_in=1024, num_heads=4)          # constructs with the reference's extra modules
    assert "gab_blocks.0.project_forward.ln0.weight" in ln.state_dict() and tuple(ln.gab_blocks[0].latent.shape) == (1, 2, 256)


def test_cpu_bag_and_unsupported_configurations_raise():
    from vlsa_amd import VlsaNativeError
    with pytest.raises(VlsaNativeError):
        _quiet()(torch.randn(1, 10, 512))
    for kw, d in (({"dim_in": 1024}, 1024), ({"dim_hid": 128}, 512), ({"num_heads": 4}, 512), ({"topk": 2}, 512), ({"ln": True}, 512),
                  ({"num_layers": 0}, 512)):
        with pytest.raises(VlsaNativeError, match="ILRA: the HIP kernels cover"):
            _quiet(**kw)(torch.randn(1, 10, d))


def test_the_factory_still_refuses_ilra():
    from vlsa_amd.model_utils import load_model
    with pytest.raises(NotImplementedError, match="no HIP implementation in this package"):
        load_model("DeepMIL", [512, 256, 4], network="ILRA")


def test_patch_round_trip_on_stand_in_modules(monkeypatch):
    from vlsa_amd.deepmil import ILRA
    from vlsa_amd.model_utils import patch_reference_ilra, unpatch_reference_ilra
    mods = {}
    for full in ("model", "model.deepmil", "model.utils"):
        mods[full] = types.ModuleType(full)
        monkeypatch.setitem(sys.modules, full, mods[full])
        if "." in full:
            setattr(mods["model"], full.split(".")[1], mods[full])
    original = type("Original", (), {})
    mods["model.deepmil"].ILRA = original                      # model.utils has none: absent before
    saved = patch_reference_ilra()
    assert mods["model.deepmil"].ILRA is ILRA and mods["model.utils"].ILRA is ILRA
    unpatch_reference_ilra(saved)
    assert mods["model.deepmil"].ILRA is original and not hasattr(mods["model.utils"], "ILRA")


@pytest.mark.skipif(not os.path.isdir("/root/reference/model"), reason="needs the upstream reference at /root/reference")
def test_patch_round_trip_on_the_reference_and_its_factory_builds_ours():
    from _ref_import import import_reference
    from vlsa_amd.deepmil import ILRA
    from vlsa_amd.model_utils import patch_reference_ilra, unpatch_reference_ilra
    import_reference()
    import model.deepmil as ref_mil
    import model.utils as ref_utils
    before = (ref_mil.ILRA, ref_utils.ILRA)
    saved = patch_reference_ilra()
    try:
        assert ref_mil.ILRA is ILRA and ref_utils.ILRA is ILRA
        with contextlib.redirect_stdout(io.StringIO()):
            built = ref_utils.load_model("DeepMIL", [512, 256, 4], network="ILRA")
    finally:
        unpatch_reference_ilra(saved)
    assert (ref_mil.ILRA, ref_utils.ILRA) == before and type(built) is ILRA and built.classifier.out_features == 4


@pytest.fixture(scope="module")
def lib():
    from vlsa_amd import build, _native
    build.build_native()
    return _native.load()


def test_tables_and_workspace_sizes_depend_on_the_row_counts_alone(lib):
    assert lib.vlsa_ilra_tile_rows() == 32 and lib.vlsa_ilra_pool_part_rows() == 256
    assert [lib.vlsa_ilra_pool_parts(n) for n in (0, 1, 256, 257, 2798, 50000, 10 ** 7)] == [1, 1, 1, 2, 11, 64, 64]
    assert lib.vlsa_ilra_pool_workspace_bytes(11, 512) == 11 * (32 + 16 * 512) * 4 and lib.vlsa_ilra_pool_workspace_bytes(11, 256) == 11 * (32 + 16 * 256) * 4
    assert lib.vlsa_ilra_pool_workspace_bytes(0, 512) == 0 and lib.vlsa_ilra_pool_workspace_bytes(4, 384) == 0
    assert lib.vlsa_ilra_rowmap_backward_workspace_bytes(100, 4, 2, 512) == (100 * 256 * 4 + 1 * 256 * 512 + 2 * 3 * 8 * 256) * 4
    assert lib.vlsa_ilra_rowmap_backward_workspace_bytes(10 ** 6, 40000, 64, 256) == (10 ** 6 * 256 * 4 + 64 * 256 * 256 + 64 * 3 * 8 * 256) * 4
    assert lib.vlsa_ilra_rowmap_backward_workspace_bytes(0, 4, 2, 512) == 0 and lib.vlsa_ilra_rowmap_backward_workspace_bytes(9, 4, 65, 512) == 0


def test_the_part_table_formula_is_the_library_function(lib):
    rows, cap = lib.vlsa_ilra_pool_part_rows(), lib.vlsa_ilra_pool_parts(1 << 62)
    ns = [1, 2, rows - 1, rows, rows + 1, 2798, cap * rows - 1, cap * rows, cap * rows + 1, 50000, 10 ** 7, 2 ** 40]
    got = torch.clamp(torch.div(torch.tensor(ns) + (rows - 1), rows, rounding_mode="floor"), 1, cap).tolist()
    assert got == [lib.vlsa_ilra_pool_parts(n) for n in ns]


P = ctypes.c_void_p(0x1000)      # any non-null address: every call below must be refused before anything is dereferenced or launched


def _pool_fwd(lib, B=2, D=512, P_=8, desc=P, tab=P, n=4, off=P, xp=None, E=P, ws=P, out=P, dt=1, **_):
    return lib.vlsa_ilra_pool_forward_batch(desc, B, dt, D, P_, tab, n, off, xp, E, ws, out, P, P, None)


def _pool_bwd(lib, B=2, D=512, P_=8, desc=P, tab=P, n=4, off=P, xp=None, E=P, ws=P, out=P, dt=1, dX=None, **_):
    return lib.vlsa_ilra_pool_backward_batch(desc, B, dt, D, P_, tab, n, off, xp, E, P, P, P, P, ws, out, dX, None)


def _rm_fwd(lib, B=2, D=512, H=256, desc=P, tab=P, n=4, off=P, xp=None, E=P, out=P, dt=1, **_):
    return lib.vlsa_ilra_rowmap_forward_batch(desc, B, dt, D, H, tab, n, off, xp, E, P, P, P, P, P, out, None, None)


def _rm_bwd(lib, B=2, D=512, H=256, desc=P, tab=P, n=4, off=P, xp=None, E=P, ws=P, out=P, dt=1, dX=None, total=100, **_):
    return lib.vlsa_ilra_rowmap_backward_batch(desc, B, dt, D, H, tab, n, off, xp, total, E, P, P, P, P, P, P, P, P, P, P, ws, out, P, P, P, P, P,
                                               dX, None)


@pytest.mark.parametrize("call", [_pool_fwd, _pool_bwd, _rm_fwd, _rm_bwd])
def test_bad_arguments_are_refused_on_the_host(lib, call):
    for kw in ({"B": 0}, {"B": 65}, {"desc": None}, {"tab": None}, {"n": 1}, {"off": None}, {"E": None}, {"out": None}):
        assert call(lib, **kw) == -1, (call.__name__, kw)
    for kw in ({"D": 256}, {"D": 1024}, {"dt": 7}, {"xp": P}, {"xp": P, "D": 256, "dt": 1}):          # packed rows are fp32 with D = 256
        assert call(lib, **kw) == -2, (call.__name__, kw)
    if call in (_pool_fwd, _pool_bwd):
        assert call(lib, P_=0) == -1 and call(lib, P_=17) == -2 and call(lib, ws=None) == -1
    else:
        assert call(lib, H=128) == -2
    if call in (_pool_bwd, _rm_bwd):
        assert call(lib, dX=P) == -1          # bag rows never receive a gradient
    if call is _rm_bwd:
        assert call(lib, total=0) == -1 and call(lib, ws=None) == -1
