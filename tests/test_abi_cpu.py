"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports exactly the symbols the header
declares, the binding derived from the header types them as the header says, and the product path refuses CPU
tensors loudly (no fallback)."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint32, c_void_p

import pytest
import torch

from abi_helpers import HEADER_PATH, declared_symbols


def test_library_builds_and_exports_every_declared_symbol():
    from vlsa_amd import build, _native
    build.build_native()
    lib = _native.load()
    declared = declared_symbols()
    assert declared, "no declarations parsed from include/vlsa_hip.h"
    for name in declared:
        assert hasattr(lib, name), f"libvlsa_hip.so does not export {name}"
    assert set(_native.exported_symbols()) == set(declared), "binding and header disagree"
    assert lib.vlsa_abi_version() == _native.ABI_VERSION


def test_host_side_queries_need_no_gpu():
    from vlsa_amd import _native
    lib = _native.load()
    assert lib.vlsa_num_partials(0) == 1
    assert lib.vlsa_num_partials(1) == 1
    assert lib.vlsa_num_partials(33) == 2
    assert lib.vlsa_num_partials(50_000) == 256
    assert lib.vlsa_qprep_bytes(512) == 16 * 512 * 4 + 3 * 16 * 512 * 2 + 17 * 512 * 4 + 128
    assert lib.vlsa_error_string(-1) == b"invalid argument"
    # tile geometry of the attention-score kernel (what the batched caller sizes its tile table with)
    for dt in (_native.DT_BF16, _native.DT_F32):
        for gated in (0, 1):
            mr, rt = ctypes.c_int(0), ctypes.c_int(0)
            assert lib.vlsa_gated_scores_tiling(dt, gated, ctypes.addressof(mr), ctypes.addressof(rt)) == 0
            assert mr.value in (64, 128, 256) and rt.value >= 64
    assert lib.vlsa_gated_scores_tiling(99, 0, ctypes.addressof(mr), ctypes.addressof(rt)) != 0
    # the persistent LDS-DMA score kernel: where it applies, and the tiling of a single-bag scores + pooling launch (host arithmetic):
    # the tiles of 256 walkers cover the bag with heights of 16 .. 256 rows whose per-walker sums differ by at most one 16-row unit
    rows, mn = ctypes.c_int(0), ctypes.c_int64(0)
    assert lib.vlsa_gated_scores_big_tile(_native.DT_BF16, 1, ctypes.addressof(rows), ctypes.addressof(mn)) == 0
    assert rows.value in (0, 256) and (rows.value == 0 or mn.value >= 1)       # (0: switched off in a -DVLSA_EXPERIMENT build)
    assert lib.vlsa_gated_scores_big_tile(_native.DT_F32, 1, ctypes.addressof(rows), ctypes.addressof(mn)) == 0 and rows.value == 0
    assert lib.vlsa_gated_scores_pool_ws_floats(0) == 0
    for N in (1, 31, 32, 33, 8191, 8192, 8193, 16384, 50_000, 65_536, 65_537, 393_216, 400_000, 4_000_000):
        ws = lib.vlsa_gated_scores_pool_ws_floats(N)
        units = -(-N // (16 * 256))                 # 16-row units per walker
        rounds = -(-units // 16)
        lo, hi = (units // rounds) * 16, -(-units // rounds) * 16      # the two tile heights of the plan
        assert 16 <= lo <= hi <= 256
        assert ws >= 514 * -(-N // hi), (N, ws, hi)                  # one (m, l, acc[512]) record per tile of the bf16 route
        assert ws >= 544 * lib.vlsa_pool_num_partials(N) + 32        # (pm, pl, pacc) + (m2, l) of the chained fp32 route
        assert ws <= max(514 * min(-(-N // lo), rounds * 256), 544 * lib.vlsa_pool_num_partials(N) + 64)


def test_default_build_reads_no_environment():
    """SURVEY.md 8(b) / include/vlsa_hip.h: "no global state".  The A/B switches of the measurement tools (VLSA_GS_*, VLSA_TT_*,
    VLSA_MAX_PARTIALS, VLSA_EXP ...) exist only in a -DVLSA_EXPERIMENT build: the default library neither imports getenv nor carries
    any of their names."""
    from vlsa_amd import build
    if os.environ.get("VLSA_EXTRA_HIPCC_FLAGS") or os.environ.get("VLSA_HIP_LIB"):
        pytest.skip("not the default build")
    lib = build.build_native()
    blob = open(lib, "rb").read()
    assert b"getenv" not in blob
    names = sorted(set(re.findall(rb"VLSA_[A-Z0-9_]{2,}", blob)))
    assert names == [], names
    nm = subprocess.run(["nm", "-D", "--undefined-only", lib], capture_output=True, text=True)
    if nm.returncode == 0:
        assert "getenv" not in nm.stdout


def test_cpu_tensor_is_refused_loudly():
    from vlsa_amd import VlsaNativeError, functional as F
    X = torch.randn(8, 512)
    Q = torch.randn(4, 512)
    with pytest.raises(VlsaNativeError):
        F.vlfan_aggregate(X, Q)


# ---- the binding is derived from include/vlsa_hip.h: what the reader makes of it, and what it refuses ----
V, I = c_void_p, c_int
SPOT_SIGNATURES = {            # one entry per rule of the type mapping, typed by hand from the declarations (never pasted from the reader's output)
    "vlsa_abi_version": (I, []),                                                            # (void)
    "vlsa_error_string": (c_char_p, [I]),                                                   # const char* return
    "vlsa_qprep_qeff": (V, [V, I]),                                                         # any other pointer return
    "vlsa_qprep_bytes": (c_size_t, [I]),
    "vlsa_gated_scores_pool_ws_floats": (c_int64, [c_int64]),
    "vlsa_adam_step": (I, [V, I, V, V, c_double, c_double, c_double, V]),                   # struct pointer, three doubles
    "vlsa_attn_scores_backward": (I, [V, I, I, I, V, I, V, I, V, V, V, V, V, c_float, c_uint32, V]),
    "vlsa_dsmil_state_floats": (c_size_t, [I, I, V]),                                       # the offsets9 out-array
    "vlsa_tt_workspace_bytes": (c_size_t, [V, V, I]),                                       # two struct pointers
    "vlsa_xchg_put": (I, [I, V, V, V, V, V, V, c_uint32, c_uint32, c_int64, V, V]),
}


@pytest.mark.parametrize("name", sorted(SPOT_SIGNATURES))
def test_derived_signature_equals_the_hand_typed_one(name):
    from vlsa_amd import _native
    assert _native._SIGNATURES[name] == SPOT_SIGNATURES[name]


def test_the_longest_derived_signature():
    from vlsa_amd import _native
    res, args = _native._SIGNATURES["vlsa_ilra_rowmap_backward_batch"]
    assert res is I and len(args) == 30
    assert args[:10] == [V, I, I, I, I, V, I, V, V, c_int64]


def test_reader_accepts_the_forms_the_header_uses():
    from vlsa_amd import _native
    consts, structs, sigs = _native.read_header("""
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define VLSA_TEN 10
        #define VLSA_HEX 0x100      /* a trailing comment */
        #define VLSA_NEG (-2)
        #define VLSA_GUARD_H
        int vlsa_a(const float* x,   /* [n] rows */
                   int n,
                   unsigned int seed,
                   int64_t off[9]);
        int vlsa_b(void);
        #ifdef __cplusplus
        }
        #endif
    """)
    assert consts == {"TEN": 10, "HEX": 256, "NEG": -2} and structs == {}
    assert sigs == {"vlsa_a": (I, [V, I, c_uint32, V]), "vlsa_b": (I, [])}


@pytest.mark.parametrize("text", [
    "int vlsa_f(short n);",                                                     # a scalar outside the type table
    "short vlsa_f(int n);",
    "typedef struct vlsa_s { int a; } vlsa_s;\nint vlsa_f(vlsa_s s);",         # a struct by value
    "typedef struct vlsa_s { int a; } vlsa_s;\nvlsa_s vlsa_f(int n);",
    "int vlsa_f(int (*done)(int), void* stream);",                              # a function-pointer parameter
    "int vlsa_f(const char* fmt, ...);",                                        # variadic
    "int vlsa_f();",
    "static int n = vlsa_foo(3);",                                              # a vlsa_foo( that is no prototype
    "vlsa_foo(3)",
    "int vlsa_f(int n);\nint vlsa_f(int n);",                                  # declared twice
    "typedef struct vlsa_s { short a; } vlsa_s;",                               # struct members outside the table
    "typedef struct vlsa_s { float a[4]; } vlsa_s;",
    "typedef struct vlsa_s { int a; } vlsa_t;",
    "struct vlsa_s { int a; };",                                                # a struct in another form
    "typedef struct vlsa_s { struct { int a; } in; } vlsa_s;",
])
def test_reader_refuses_what_it_would_have_to_guess(text):
    from vlsa_amd import _native
    with pytest.raises(_native.VlsaNativeError):
        _native.read_header(text)


def test_derived_structs_have_the_compilers_layout(tmp_path):
    from vlsa_amd import _native, prompt_encoder
    names = ["vlsa_bag_desc", "vlsa_rows_desc", "vlsa_adam_tensor", "vlsa_tt_layer", "vlsa_tt_model", "vlsa_tt_rows"]
    assert sorted(_native.STRUCTS) == sorted(names)
    sizes = [ctypes.sizeof(_native.STRUCTS[n]) for n in names]
    assert sizes[:4] == [24, 16, 48, 96]
    assert prompt_encoder._TTLayer is _native.STRUCTS["vlsa_tt_layer"] and prompt_encoder._TTModel is _native.STRUCTS["vlsa_tt_model"]
    assert prompt_encoder._TTRows is _native.STRUCTS["vlsa_tt_rows"] and _native.AdamTensor is _native.STRUCTS["vlsa_adam_tensor"]
    assert _native.STRUCTS["vlsa_tt_model"].layer.size == ctypes.sizeof(c_void_p)           # POINTER(vlsa_tt_layer): one pointer
    cc = next((c for c in map(shutil.which, ("cc", "gcc", "clang", "hipcc")) if c), None) or "/opt/rocm/bin/hipcc"
    if not os.path.exists(cc):
        pytest.skip("no C compiler to ask for the struct sizes")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "vlsa_hip.h"\nint main(void) { printf("'
                   + " ".join(["%zu"] * len(names)) + '\\n", ' + ", ".join(f"sizeof({n})" for n in names) + "); return 0; }\n")
    lang = ["-x", "c++"] if os.path.basename(cc) == "hipcc" else []                          # hipcc in host mode
    subprocess.run([cc, *lang, "-I", os.path.dirname(HEADER_PATH), str(src), "-o", str(tmp_path / "sizes")], check=True)
    out = subprocess.run([str(tmp_path / "sizes")], check=True, capture_output=True, text=True).stdout
    assert sizes == [int(x) for x in out.split()]


def test_library_defines_no_entry_point_the_header_does_not_declare():
    """the converse of test_library_builds_and_exports_every_declared_symbol: an extern "C" vlsa_* defined in a .hip file but
    not declared gets no compiler check against the header and no binding"""
    from vlsa_amd import build
    if os.environ.get("VLSA_EXTRA_HIPCC_FLAGS") or os.environ.get("VLSA_HIP_LIB"):
        pytest.skip("not the default build")             # (a -DVLSA_EXPERIMENT build adds the measurement tools' read-back calls)
    if not shutil.which("nm"):
        pytest.skip("no nm")
    nm = subprocess.run(["nm", "-D", "--defined-only", build.build_native()], capture_output=True, text=True, check=True)
    defined = {line.split()[-1] for line in nm.stdout.splitlines() if line.split() and line.split()[-1].startswith("vlsa_")}
    assert defined == set(declared_symbols())


def test_status_codes_come_from_the_header():
    from vlsa_amd import _native
    assert (_native.OK, _native.EINVAL, _native.EUNSUPPORTED, _native.ELAUNCH) == (0, -1, -2, -3)
