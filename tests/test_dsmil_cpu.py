"""DSMIL and the SA-baseline factory, the parts that need no GPU: state-dict keys against the fixtures' key list, ``load_model('DeepMIL',
dims, network=...)`` for the served networks, the ``patch_reference`` round trip of the three new names, the C ABI's declarations and
host-side argument checks, the refusal of DSMIL as a VLSA image encoder and of CPU input."""
import ctypes
import glob
import os
import sys
import types

import numpy as np
import pytest
import torch

import dsmil_cases as DC
from abi_helpers import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vlsa_dsmil_parts", "vlsa_dsmil_workspace_bytes", "vlsa_dsmil_state_floats", "vlsa_dsmil_forward_batch", "vlsa_dsmil_backward_batch")


def test_state_dict_keys_and_shapes_equal_the_fixtures():
    from vlsa_amd.deepmil import DSMIL
    gold = os.path.join(ROOT, "tests", "golden")
    assert sorted(glob.glob(os.path.join(gold, "dsmil_*.npz"))) == sorted(
        os.path.join(gold, f"dsmil_{n}{tag}.npz") for n in DC.CASES for tag in ("", "_gq", "_gv"))
    for name in DC.CASES:
        fx = np.load(os.path.join(gold, f"dsmil_{name}.npz"))
        for k, tag in DC.BIG.items():
            assert np.load(os.path.join(gold, f"dsmil_{name}_{tag}.npz"))["grad"].shape == tuple(fx["shape/" + k]) == (256, 512)
        C, fp = DC.CASES[name][1], DC.CASES[name][5]
        m = DSMIL(dim_in=512, dim_hid=256, num_cls=C, use_feat_proj=fp, drop_rate=0.25)
        sd = m.state_dict()
        assert [k for k in sd if not k.startswith("feat_proj.")] == list(fx["keys"])
        assert [k for k in sd if k.startswith("feat_proj.")] == (list(DC.FP_KEYS) if fp else [])
        for k in fx["keys"]:
            assert tuple(sd[k].shape) == tuple(fx["shape/" + k]), k


def test_load_model_builds_the_served_baselines_and_names_what_the_others_miss():
    from vlsa_amd.deepmil import DSMIL, DeepMIL
    from vlsa_amd.layers import Attention_Pooling, Gated_Attention_Pooling
    from vlsa_amd.model_utils import load_model
    dims = [512, 256, 4]
    m = load_model("DeepMIL", dims, network="ABMIL", use_feat_proj=False)
    assert type(m) is DeepMIL and isinstance(m.sigma, Attention_Pooling) and m.g.out_features == 4
    m = load_model("DeepMIL", dims, network="ABMIL", pooling="gated_attention", use_feat_proj=False)
    assert isinstance(m.sigma, Gated_Attention_Pooling)
    with pytest.raises(AssertionError):
        load_model("DeepMIL", dims, network="ABMIL", pooling="max")
    for net, pooling in (("MaxMIL", "max"), ("MeanMIL", "mean")):
        m = load_model("DeepMIL", dims, network=net, use_feat_proj=False)
        assert type(m) is DeepMIL and m.sigma == pooling
        with pytest.raises(AssertionError):
            load_model("DeepMIL", dims, network=net, pooling="attention")
    m = load_model("DeepMIL", dims, network="DSMIL", use_feat_proj=True, drop_rate=0.1)
    assert type(m) is DSMIL and m.feat_proj is not None and m.b_classifier.v[0].p == 0.1
    assert m.i_classifier.fc[0].out_features == 4 and tuple(m.b_classifier.fcc.weight.shape) == (4, 4, 256)
    for net, need in (("TransMIL", "nystrom_attention"), ("ILRA", "nystrom_attention"), ("PatchGCN", "torch_geometric"), ("DeepAttnMISL", "cluster")):
        with pytest.raises(NotImplementedError, match=need):
            load_model("DeepMIL", dims, network=net)
    with pytest.raises(AssertionError):
        load_model("DeepMIL", dims)


def test_dsmil_is_refused_as_a_vlsa_image_encoder_with_the_reason():
    from vlsa_amd.vlsa import build_mil_encoder
    with pytest.raises(ValueError, match="class logits"):
        build_mil_encoder(dict(name="DSMIL", dim_in=512, dim_hid=256))


def test_cpu_input_and_unsupported_widths_raise():
    from vlsa_amd._native import VlsaNativeError
    from vlsa_amd.deepmil import DSMIL
    m = DSMIL(dim_in=512, dim_hid=256, num_cls=4, use_feat_proj=False).eval()
    with pytest.raises(VlsaNativeError):
        m(torch.randn(1, 10, 512))
    with pytest.raises(VlsaNativeError):
        DSMIL(dim_in=1024, dim_hid=256, num_cls=4, use_feat_proj=False)(torch.randn(1, 10, 1024))


def _stand_ins(monkeypatch, names):
    mods = {}
    for name in names:
        parts = name.split(".")
        for k in range(1, len(parts) + 1):
            full = ".".join(parts[:k])
            if full not in mods:
                mods[full] = types.ModuleType(full)
                monkeypatch.setitem(sys.modules, full, mods[full])
                if k > 1:
                    setattr(mods[".".join(parts[:k - 1])], parts[k - 1], mods[full])
    return mods


def _round_trip(ref_utils, ref_mil):
    from vlsa_amd import deepmil as fast
    from vlsa_amd.model_utils import patch_reference, unpatch_reference
    before = (ref_utils.DeepMIL, ref_utils.DSMIL, ref_mil.DSMIL)
    saved = patch_reference()
    try:
        assert (ref_utils.DeepMIL, ref_utils.DSMIL, ref_mil.DSMIL) == (fast.DeepMIL, fast.DSMIL, fast.DSMIL)
        built = ref_utils.load_model("DeepMIL", [512, 256, 4], network="DSMIL", use_feat_proj=False) if hasattr(ref_utils, "load_model") else None
    finally:
        unpatch_reference(saved)
    assert (ref_utils.DeepMIL, ref_utils.DSMIL, ref_mil.DSMIL) == before
    return built


def test_patch_reference_round_trip_on_stand_in_modules(monkeypatch):
    mods = _stand_ins(monkeypatch, ["model.utils", "model.vlsa", "model.deepmil"])
    for mod, attrs in (("model.utils", ("VLSA", "DeepMIL", "DSMIL")), ("model.vlsa", ("VLSA", "logit_pooling")),
                       ("model.deepmil", ("VLFAN", "FeatMIL", "DeepMIL", "DSMIL", "logit_pooling"))):
        for a in attrs:
            setattr(mods[mod], a, type("Original_" + a, (), {}))
    _round_trip(mods["model.utils"], mods["model.deepmil"])


@pytest.mark.skipif(not os.path.isdir("/root/reference/model"), reason="needs the upstream reference at /root/reference")
def test_patch_reference_round_trip_on_the_reference_and_its_factory_builds_ours():
    from _ref_import import import_reference
    from vlsa_amd import deepmil as fast
    import_reference()
    import model.deepmil as ref_mil
    import model.utils as ref_utils
    built = _round_trip(ref_utils, ref_mil)
    assert type(built) is fast.DSMIL          # the reference's own load_model, unmodified, on the patched names


@pytest.fixture(scope="module")
def lib():
    from vlsa_amd import build, _native
    build.build_native()
    return _native.load()


def test_new_symbols_exported_declared_and_bound(lib):
    from vlsa_amd import _native
    declared = set(declared_symbols())
    assert declared == set(_native.exported_symbols())           # header == bindings still holds
    for name in NEW:
        assert hasattr(lib, name) and name in declared


def test_parts_depend_on_the_row_count_alone_and_sizes_are_consistent(lib):
    assert [lib.vlsa_dsmil_parts(n) for n in (0, 1, 512, 513, 2798, 50000, 10 ** 7)] == [1, 1, 1, 2, 6, 64, 64]
    off = (ctypes.c_int64 * 9)()
    total = lib.vlsa_dsmil_state_floats(3, 4, off)
    assert list(off)[:4] == [0, 48, 96, 144] and total == 192 + 3 * 4 * (512 * 3 + 256 * 2)
    assert lib.vlsa_dsmil_workspace_bytes(10, 4) > 10 * 4 * 512 * 4
    assert lib.vlsa_dsmil_workspace_bytes(0, 4) == 0 and lib.vlsa_dsmil_state_floats(1, 17, None) == 0


P = ctypes.c_void_p(0x1000)      # any non-null address: every call below must be refused before anything is dereferenced or launched


def _fwd(lib, B=2, D=512, H=256, C=4, desc=P, ps=P, n_parts=4, Wc=P, drop=0.0, seed=P, ws=P, state=P, logits=P, attn=None, aoff=None, dt=1):
    return lib.vlsa_dsmil_forward_batch(desc, B, dt, D, H, C, ps, n_parts, Wc, P, P, P, P, P, P, P, drop, seed, ws, state, logits, attn,
                                        aoff, None)


def _bwd(lib, B=2, D=512, H=256, C=4, desc=P, ps=P, n_parts=4, Wq=P, drop=0.0, seed=P, state=P, ws=P, dWc=P, dt=1, g=P):
    return lib.vlsa_dsmil_backward_batch(desc, B, dt, D, H, C, ps, n_parts, Wq, P, P, g, drop, seed, state, ws, dWc, P, P, P, P, P, P, P,
                                         None)


@pytest.mark.parametrize("call", [_fwd, _bwd])
def test_bad_arguments_are_refused_on_the_host(lib, call):
    for kw in ({"B": 0}, {"B": 65}, {"desc": None}, {"ps": None}, {"n_parts": 1}, {"C": 0}, {"drop": 1.0}, {"drop": -0.1},
               {"drop": 0.25, "seed": None}, {"ws": None}, {"state": None}):
        assert call(lib, **kw) == -1, (call.__name__, kw)
    for kw in ({"D": 256}, {"D": 1024}, {"H": 128}, {"C": 17}, {"dt": 7}):
        assert call(lib, **kw) == -2, (call.__name__, kw)
    assert _fwd(lib, Wc=None) == -1 and _fwd(lib, logits=None) == -1 and _fwd(lib, attn=P, aoff=None) == -1
    assert _bwd(lib, Wq=None) == -1 and _bwd(lib, g=None) == -1 and _bwd(lib, dWc=None) == -1
