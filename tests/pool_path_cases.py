"""Cases, input recipes and float64 references for the single-bag pooling kernels of vlsa_amd/csrc/mil_pool.hip: scored pooling and
its backward, column max, row dots and normalize_many.  Plain torch-CPU: nothing here touches a GPU or the native library.

The single-bag entry points choose a kernel at run time from the feature width D, the row stride and the pointer alignment
(launch_scored, launch_colmax, rowdot_impl, vlsa_normalize_many).  ``expected_path`` restates those predicates; ``CASES`` names at
least one case for every instantiation the library can reach, at the row counts where the 4-row unroll, the waves of a workgroup and
the partial count change, and at the 512-partial cap.

Unreachable on purpose: the bf16 NC = 3 and NC = 4 instantiations of k_scored_pool_partial_vec and k_colmax_partial_vec.  A bf16
lane reads 8 values per 16-byte chunk, so NC = 3 needs D > 1024 = VLSA_MAX_D, which the entry points refuse.  No case tries.

A case is ``(entry, dtype, N, D, ldx, byte_offset, kind)``: ``ldx`` in elements (``ldx == D``: contiguous), ``byte_offset`` the
misalignment of the first element against a 16-byte boundary, ``kind`` the input recipe (``make_inputs``).
"""
import zlib

import torch

MAX_D = 1024                       # VLSA_MAX_D
ESZ = {"f32": 4, "bf16": 2}
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}
ENTRIES = ("scored_pool", "colmax", "rowdot", "pool_backward", "normalize")
SENTINEL = 3.0e4                   # fills the rows and columns of a base tensor that a view leaves out (exact in bf16's range)

# ---- gates: what the suite already asserts for these kernels ------------------------------------------------------------------------
GATE_POOL = 1e-5                   # x max(1, max|ref|)   test_streaming_reductions_vs_torch
GATE_ROWDOT = 2e-5                 # x max(1, max|ref|)   the same test
GATE_NORMALIZE = 8e-7              # absolute             test_normalize_many
GATE_TOPK = 2e-6                   # x max(1, max|ref|)   test_topk_mean_two_stage
GATE_BACKWARD = 1e-4               # of the reference's largest entry: check_grads in deepattnmisl_helpers.py
GATE_QPOOL = 1e-4                  # TOL of test_gpu_gated_scores.py


def _nc(dtype, D):
    return (D + 64 * (16 // ESZ[dtype]) - 1) // (64 * (16 // ESZ[dtype]))


def expected_path(entry, dtype, D, ldx, byte_offset, out_offset=0):
    """The kernel family and instantiation the library chooses: ("vec", NC) / ("scalar", DPL) (DPL 0: k_rowdot has none), or the
    refusal "unsupported" / "einval".  out_offset: misalignment of normalize_many's output pointer."""
    esz = ESZ[dtype]
    vec = 16 // esz
    fast = D % vec == 0 and (ldx * esz) % 16 == 0 and byte_offset % 16 == 0
    if entry in ("scored_pool", "colmax"):
        if D > MAX_D:
            return "einval"
        if fast:
            return ("vec", _nc(dtype, D))
        return ("scalar", 4 if D <= 256 else 8 if D <= 512 else 12 if D <= 768 else 16)
    if entry in ("rowdot", "pool_backward"):
        if fast and D <= MAX_D:
            return ("vec", _nc(dtype, D))
        return "unsupported" if entry == "pool_backward" else ("scalar", 0)
    if entry == "normalize":
        if D > MAX_D:
            return "einval"
        if not fast or D % 4 or out_offset % 16:
            return "unsupported"
        return ("vec", _nc(dtype, D))
    raise ValueError(entry)


def case_path(case):
    entry, dtype, N, D, ldx, off, kind = case
    return expected_path(entry, dtype, D, ldx, off, out_offset=4 if kind == "misaligned_out" else 0)


# ---- the case list ------------------------------------------------------------------------------------------------------------------
ROWS = (1, 3, 5, 63, 64, 65, 127, 129, 257)     # a wave without rows; a last 4-row group of 1 / 2 / 3 rows; one -> two partials
ROWS_KINDS = (5, 65, 257)                       # the rows the recipes other than randn run at (neg_inf_rows: 6 for 5)
ROWS_CAP = (32_704, 32_705, 32_768, 32_773, 33_000)   # last N below the 512-partial cap, first at it, shares of 64, five of 65, no multiple of 4
SCALAR_WIDTHS = {"f32": (1, 65, 255, 257, 511, 513, 767, 769, 1023), "bf16": (4, 100, 260, 516, 1020)}
VECTOR_WIDTHS = {"f32": (4, 256, 260, 512, 516, 768, 772, 1024), "bf16": (8, 264, 512, 520, 1024)}
ODD_STRIDE = {"f32": 513, "bf16": 516}          # a row stride that is no multiple of 16 bytes
POOL_KINDS = ("spike_last", "spike_first", "one_hot", "flat", "neg_inf_rows", "big_rows")


def _layouts(dtype):
    """(D, ldx, byte_offset) of every layout of the scored-pool / colmax / rowdot entry points"""
    out = [(D, D, 0) for D in SCALAR_WIDTHS[dtype]]
    out += [(512, ODD_STRIDE[dtype], 0), (512, 512, ESZ[dtype])]                # scalar by stride, by pointer
    out += [(D, D, 0) for D in VECTOR_WIDTHS[dtype]]
    out += [(512, 640, 0), (512, 1024, 0)]                                      # vector kernels with ldx != D
    return out


def _kind_layouts(dtype):
    """the layouts the other recipes run at: a scalar and a vector kernel by width, D = 512 on both paths, the widest vector one"""
    w = {"f32": [(513, 513, 0), (772, 772, 0)], "bf16": [(516, 516, 0), (520, 520, 0)]}[dtype]
    return w + [(512, 512, 0), (512, ODD_STRIDE[dtype], 0), (512, 640, 0)]


def _rows_of(kind):
    return tuple(6 if (kind == "neg_inf_rows" and n == 5) else n for n in ROWS_KINDS)


def _build_cases():
    cases = []
    add = lambda *c: cases.append(tuple(c))  # noqa: E731
    for dtype in ("f32", "bf16"):
        for entry, kinds in (("scored_pool", POOL_KINDS), ("colmax", ("spike_last", "spike_first", "ties", "big_rows")),
                             ("rowdot", ("big_rows",))):
            lay = _layouts(dtype) + ([(1028, 1028, 0)] if entry == "rowdot" and dtype == "f32" else [])
            for D, ldx, off in lay:
                for N in ROWS:
                    add(entry, dtype, N, D, ldx, off, "randn")
            for D, ldx, off in _kind_layouts(dtype):
                for kind in kinds:
                    for N in _rows_of(kind):
                        add(entry, dtype, N, D, ldx, off, kind)
            for ldx in (512, ODD_STRIDE[dtype]):                                 # at the partial cap: D = 512, both paths
                for N in ROWS_CAP:
                    add(entry, dtype, N, 512, ldx, 0, "randn")
                for kind in (kinds if dtype == "f32" else kinds[:1]):
                    add(entry, dtype, 32_773, 512, ldx, 0, kind)
        # the fused backward: vector kernels only; the scalar conditions are refused
        for D, ldx, off in [(D, D, 0) for D in VECTOR_WIDTHS[dtype]] + [(512, 640, 0), (512, 1024, 0)]:
            for N in ROWS:
                add("pool_backward", dtype, N, D, ldx, off, "randn")
        for kind in ("one_hot", "neg_inf_rows"):      # (a spike row is no case here: x_n . v - pooled . v cancels in fp32, torch's too)
            for N in _rows_of(kind):
                add("pool_backward", dtype, N, 512, 512, 0, kind)
                add("pool_backward", dtype, N, 512, 640, 0, kind)
        for N in ROWS_CAP:
            add("pool_backward", dtype, N, 512, 512, 0, "randn")
        for D, ldx, off in [(SCALAR_WIDTHS[dtype][-1],) * 2 + (0,), (512, ODD_STRIDE[dtype], 0), (512, 512, ESZ[dtype])]:
            add("pool_backward", dtype, 65, D, ldx, off, "randn")                # VLSA_EUNSUPPORTED
        # normalize_many
        for D in {"f32": (4, 256, 260, 516, 772, 1024), "bf16": (8, 264, 520, 1024)}[dtype]:
            for N in ROWS:
                add("normalize", dtype, N, D, D, 0, "randn")
            add("normalize", dtype, 65, D, D, 0, "tiny_rows")
        for N in (5, 65, 257):
            add("normalize", dtype, N, 512, 640, 0, "randn")
            add("normalize", dtype, N, 512, 640, 0, "tiny_rows")
        add("normalize", dtype, 0, 512, 512, 0, "randn")
        add("normalize", dtype, 5, {"f32": 6, "bf16": 12}[dtype], {"f32": 6, "bf16": 12}[dtype], 0, "randn")    # D % 4, D % VEC
        add("normalize", dtype, 5, 512, ODD_STRIDE[dtype], 0, "randn")
        add("normalize", dtype, 5, 512, 512, 8, "randn")
        add("normalize", dtype, 5, 512, 512, 0, "misaligned_out")
        add("normalize", dtype, 5, 1028, 1028, 0, "randn")                       # VLSA_EINVAL
    return cases


CASES = _build_cases()


def case_id(case):
    entry, dtype, N, D, ldx, off, kind = case
    return f"{entry}-{dtype}-N{N}-D{D}-ld{ldx}-o{off}-{kind}"


def cases_of(entry):
    return [c for c in CASES if c[0] == entry]


# ---- input recipes ------------------------------------------------------------------------------------------------------------------
_BASE = {}


def _randn_rows(N, D, seed):
    """[N, D] fp32 standard normal; the N >= 32 704 cases share one base tensor (its first N rows) instead of drawing 17M numbers each"""
    if N >= ROWS_CAP[0] and D == 512:
        if "x" not in _BASE:
            _BASE["x"] = torch.randn(ROWS_CAP[-1], 512, generator=torch.Generator().manual_seed(20_512))
        return _BASE["x"][:N].clone()
    return torch.randn(N, D, generator=torch.Generator().manual_seed(seed))


def make_inputs(case):
    """{"X": [N, D] of the case's dtype, "a": [N] fp32 raw scores, "v": [D] fp32} by the recipe ``kind``, one seeded generator per case.
    The recipes make a dropped or doubled row visible:
      randn          standard normal rows, scores 3 * normal
      spike_last     every column's maximum, and the largest score, in row N - 1          spike_first: the same in row 0
      one_hot        one score 60 above the rest: the pooled row equals that row
      flat           all scores equal: the pooled row is the mean
      neg_inf_rows   the scores of rows 0 .. 3 and N - 1 are -inf (N >= 6)
      big_rows       one row scaled by 1e4 and one by 1e-4
      ties           two rows share the maximum of column 0; the last column is all zeros of alternating sign (D >= 2)
      tiny_rows      (normalize) row 1 is zero -- the 1e-12 clamp -- and row 2 is 1e-20 throughout
    """
    entry, dtype, N, D, ldx, off, kind = case
    seed = zlib.crc32(repr(case).encode())
    g = torch.Generator().manual_seed(seed ^ 0x5bd1e995)
    X = _randn_rows(N, D, seed)
    a = torch.randn(N, generator=g) * 3
    v = torch.randn(D, generator=g)
    if kind in ("spike_last", "spike_first") and N > 0:
        r = N - 1 if kind == "spike_last" else 0
        X[r] = 8.0 + torch.rand(D, generator=g)
        a[r] = a.max() + 2.0
    elif kind == "one_hot":
        a[N // 2] = a.max() + 60.0
    elif kind == "flat":
        a[:] = 0.7
    elif kind == "neg_inf_rows":
        assert N >= 6
        a[:4] = float("-inf")
        a[N - 1] = float("-inf")
    elif kind == "big_rows":
        X[N // 3] *= 1e4
        X[(2 * N) // 3] *= 1e-4
    elif kind == "ties":
        X[N // 4, 0] = X[N - 1, 0] = 9.0
        if D >= 2:
            X[:, D - 1] = 0.0
            X[::2, D - 1] = -0.0
    elif kind == "tiny_rows":
        if N > 1:
            X[1] = 0.0
        if N > 2:
            X[2] = 1e-20
    return {"X": X.to(TORCH_DT[dtype]), "a": a, "v": v}


def embed(X, ldx, byte_offset, extra_rows=1):
    """(base, view): ``view`` holds X with row stride ldx, its first element ``byte_offset`` bytes past the (16-byte aligned) start of
    ``base``; every other element of base -- the columns past D, ``extra_rows`` rows past N -- holds SENTINEL, so that a kernel that
    reads one column or one row too many shows it.  Upload ``base`` and take the same view of the copy (``view_of``)."""
    N, D = X.shape
    skip = byte_offset // X.element_size()
    base = torch.full(((N + extra_rows) * ldx + skip,), SENTINEL, dtype=X.dtype)
    view = base[skip:skip + N * ldx].view(N, ldx)[:, :D] if N > 0 else base[:0].view(0, D)
    view.copy_(X)
    return base, view


def view_of(base, N, D, ldx, byte_offset):
    skip = byte_offset // base.element_size()
    return torch.as_strided(base, (N, D), (ldx, 1), skip)


# ---- float64 references, from the values the kernel reads (a bf16 input widens exactly) --------------------------------------------
def softmax64(a):
    a = a.double()
    w = torch.exp(a - a.max())
    return w / w.sum()


def ref_scored_pool(X, a=None):
    X = X.double()
    return X.mean(dim=0) if a is None else softmax64(a) @ X


def ref_colmax(X):
    return X.double().max(dim=0).values


def ref_rowdot(X, v):
    return X.double() @ v.double()


def ref_scored_pool_backward(X, a, v):
    """da_n = A_n (x_n . v - pooled . v)"""
    X, v, A = X.double(), v.double(), softmax64(a)
    return A * (X @ v - (A @ X) @ v)


def ref_normalize(X):
    X = X.double()
    return X / X.norm(dim=-1, keepdim=True).clamp_min(1e-12)


def ref_topk_mean(S, k):
    return S.double().topk(min(k, S.shape[1]), dim=1).values.mean(dim=1)


def backward_scale(X, a, v):
    """What an error of the score gradient is measured against: the reference's largest entry -- unless that entry is itself rounding
    noise.  da_n = A_n g_n - A_n (pooled . v) is a difference of terms of size max |A_n g_n| (g = X v); with the whole softmax weight on
    one row it cancels to ~e^-60 of them, a relative error of an fp32 evaluation against it does not exist, and the size of the terms is
    the scale -- the rule ``grad_scale`` of deepattnmisl_helpers.py states for an identically-zero gradient, with its 1e-9 threshold."""
    ref = ref_scored_pool_backward(X, a, v)
    terms = float((softmax64(a) * (X.double() @ v.double())).abs().max())
    big = float(ref.abs().max())
    return big if big > 1e-9 * terms else terms


def stats_log2(a):
    """(m2, l) the forward hands to the backward: log2-domain maximum and the sum of exp2(a log2(e) - m2), in float64"""
    t = a.double() * 1.4426950408889634
    m2 = t.max()
    return float(m2), float(torch.exp2(t - m2).sum())
