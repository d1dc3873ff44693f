"""ctypes binding of libvlsa_hip.so -- the ONLY compute backend of this package.

There is no CPU / eager-PyTorch fallback: if the shared library is missing or a call fails, the
caller gets a ``VlsaNativeError`` immediately (the product path must fail loudly, never silently
route around the HIP kernels).
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_ubyte, c_uint32, c_void_p

_PKG = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("VLSA_HIP_LIB") or os.path.join(_PKG, "_lib", "libvlsa_hip.so")
_HEADER_PATH = os.path.normpath(os.path.join(_PKG, "..", "include", "vlsa_hip.h"))     # the file every .hip source is compiled against


class VlsaNativeError(RuntimeError):
    pass


# ---- the C ABI, read from include/vlsa_hip.h: its #defines, structs and prototypes are the only statement of it ----
# Not a C parser: it knows the few forms the header uses and refuses everything else (a guessed type is a shifted argument list).
_SCALARS = {"int": c_int, "int64_t": c_int64, "long long": c_int64, "size_t": c_size_t, "float": c_float, "double": c_double,
            "uint32_t": c_uint32, "unsigned int": c_uint32, "unsigned": c_uint32}


def _constants(text: str) -> dict:
    """{NAME: value} of every ``#define VLSA_<NAME> <integer>``: decimal, hex or a parenthesised negative"""
    found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+VLSA_(\w+)[ \t]+\(?[ \t]*(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*\)?[ \t]*$", text, flags=re.M)
    return {name: int(value, 0) for name, value in found}


def _structs(text: str):
    """({name: ctypes.Structure} of every ``typedef struct name { ... } name;``, the text without them).  A member is a scalar of the
    table or an unsigned char, a pointer to one of those or to void (c_void_p), or a pointer to an earlier struct (POINTER of it);
    one declaration may hold several declarators."""
    structs = {}
    scalars = dict(_SCALARS, **{"unsigned char": c_ubyte})

    def member(base, star):
        if star:
            return ctypes.POINTER(structs[base]) if base in structs else c_void_p if base in scalars or base == "void" else None
        return scalars.get(base)

    def one(m):
        name, body, alias = m.groups()
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            head = re.fullmatch(r"(?:const )?((?:unsigned )?\w+)\b(.*)", decl)
            items = [re.fullmatch(r" ?(\*?) ?(\w+) ?", d) for d in head.group(2).split(",")] if head else [None]
            types = [it and member(head.group(1), it.group(1)) for it in items]
            if not all(types):
                raise VlsaNativeError(f"struct {name}: no ctypes type for the member declaration '{decl}'")
            fields += [(it.group(2), t) for it, t in zip(items, types)]
        if alias != name:
            raise VlsaNativeError(f"struct {name} is typedef'd as {alias}")
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
        return " "

    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", one, text)
    if re.search(r"\bstruct\b", text):
        raise VlsaNativeError("a struct that is not written as 'typedef struct name { members } name;'")
    return structs, text


def _prototypes(text: str) -> dict:
    """{name: (restype, [argtypes])} of every ``<ret> vlsa_name(<params>);`` of a text without comments, preprocessor lines and
    structs.  Any pointer or array parameter is a c_void_p; a scalar outside the table, a struct by value, a function pointer,
    ``...`` and any other ``vlsa_name(`` are errors."""
    sigs = {}
    for stmt in text.split(";"):
        m = re.fullmatch(r"\s*([\w\s*]+?)\b(vlsa_\w+)\s*\(([^()]*)\)\s*", stmt)
        if not m:
            if re.search(r"\bvlsa_\w+\s*\(", stmt):
                raise VlsaNativeError(f"not a prototype the binding can read: '{' '.join(stmt.split())}'")
            continue
        name = m.group(2)
        ret, *params = (re.sub(r"\bconst\b", " ", t).split() for t in [m.group(1)] + m.group(3).split(","))
        if "*" in "".join(ret):
            res = c_char_p if "".join(ret) == "char*" else c_void_p
        else:
            res = _SCALARS.get(" ".join(ret))
        args = []
        for words in ([] if params == [["void"]] else params):
            if "*" in "".join(words) or "[" in "".join(words):
                args.append(c_void_p)
            else:       # the type alone, or the type and a parameter name
                args.append(_SCALARS.get(" ".join(words)) or _SCALARS.get(" ".join(words[:-1])))
        if res is None or None in args or name in sigs:
            raise VlsaNativeError(f"{name}: declared twice, or no ctypes type for its return value or a parameter: '{' '.join(stmt.split())}'")
        sigs[name] = (res, args)
    return sigs


def read_header(text: str):
    """(constants, structs, signatures) of a header text"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = _constants(text)
    structs, text = _structs(re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', " ", text, flags=re.M))
    return constants, structs, _prototypes(text)


try:
    with open(_HEADER_PATH) as _f:
        _CONSTANTS, STRUCTS, _SIGNATURES = read_header(_f.read())
except OSError as exc:
    raise VlsaNativeError(f"cannot read the C ABI header {_HEADER_PATH}: {exc}") from exc
globals().update(_CONSTANTS)        # ABI_VERSION, DT_*, KERNEL_*, POOL_*, MAX_*, TT_PERSISTENT, ADAM_MAX_TENSORS, OK, EINVAL, EUNSUPPORTED, ELAUNCH
P_STRIDE = 16                       # the header has no macro for the 16-float stride of the per-query statistics
AdamTensor = STRUCTS["vlsa_adam_tensor"]

_lib = None


def lib_path() -> str:
    return _LIB_PATH


def exported_symbols():
    """Names every build of the library must export (checked against include/vlsa_hip.h in the tests)."""
    return sorted(_SIGNATURES)


def load():
    """dlopen the library (once) and type every entry point.  Raises VlsaNativeError if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise VlsaNativeError(
            f"{_LIB_PATH} is missing: build it with `python -m vlsa_amd.build` (hipcc, gfx950). "
            "vlsa_amd has no CPU fallback.")
    try:
        lib = ctypes.CDLL(_LIB_PATH)
    except OSError as exc:  # pragma: no cover
        raise VlsaNativeError(f"cannot load {_LIB_PATH}: {exc}") from exc
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise VlsaNativeError(f"{_LIB_PATH} does not export {name}") from exc
        fn.restype = res
        fn.argtypes = args
    ver = lib.vlsa_abi_version()
    if ver != ABI_VERSION:
        raise VlsaNativeError(f"ABI mismatch: library {ver}, binding {ABI_VERSION}")
    _lib = lib
    return lib


def check(code: int, what: str):
    if code != 0:
        msg = load().vlsa_error_string(code).decode()
        raise VlsaNativeError(f"{what} failed: {msg} ({code})")


# ---- library-GEMM detours: an N-sized tensor (a bag's rows) that takes a torch route instead of a HIP kernel of this package ----
TORCH_ROUTE_ROWS = 1024          # P-sized inputs (<= 16 query rows) take torch ops by design; a bag is thousands of rows
torch_route_counts: dict = {}    # site -> number of calls with >= TORCH_ROUTE_ROWS rows (tests and benches read this)


def note_torch_route(site: str, rows: int, why: str) -> None:
    """Count -- and warn ONCE per site about -- a call that sends ``rows`` patch rows through torch library ops (rocBLAS GEMMs,
    [N, hidden] activations in HBM) because no fused kernel covers the configuration.  Correct, but several times slower than
    the HIP route and invisible otherwise."""
    if rows < TORCH_ROUTE_ROWS:
        return
    n = torch_route_counts.get(site, 0)
    torch_route_counts[site] = n + 1
    if n == 0:
        import warnings
        warnings.warn(f"vlsa_amd: {site}: {rows} patch rows go through torch library ops, not a fused HIP kernel ({why}); "
                      "further calls are counted in vlsa_amd._native.torch_route_counts", RuntimeWarning, stacklevel=3)


class TransientCaches:
    """nn.Module mixin.  The attributes named in ``_transient`` hold native handles (ctypes structures with device pointers), device
    scratch or cached results tied to them; none of it is state.  ``copy.deepcopy`` / ``pickle`` / ``torch.save(module)`` go
    through ``__getstate__``: the entries are dropped there (ctypes objects with pointers cannot even be pickled) and rebuilt on
    next use.  ``_transient`` maps a name to a zero-argument factory of its empty value, or to ``None`` = delete the attribute."""
    _transient: dict = {}

    def __getstate__(self):
        state = self.__dict__.copy()
        for name, make in self._transient.items():
            if name in state:
                if make is None:
                    del state[name]
                else:
                    state[name] = make()
        return state
