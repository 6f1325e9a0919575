"""ctypes binding of the C-ABI kernel library (include/surf_hip.h -> surf_amd/libsurf_hip.so).

The library is the product path: there is no CPU fallback.  Importing this module without the
built library raises; calling a kernel without a GPU fails inside HIP.

The header is the only place a signature or the ABI version is written: both are parsed from it at import, and lib()
makes every status-returning entry point raise SurfHipError on a non-zero status by itself.
"""
import ctypes
import os
import re
import subprocess

import torch  # noqa: F401  (load PyTorch's HIP runtime first: one runtime per process, whichever import order the caller uses)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SURF_HIP_LIB", os.path.join(_HERE, "libsurf_hip.so"))

HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "surf_hip.h"))

# every parameter spelling include/surf_hip.h uses; anything with a `*` is a pointer
_CTYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
           "double": ctypes.c_double}
_DECL_HEAD = re.compile(r"^[ \t]*(?:int|int64_t)\s+(surf_\w+)\s*\(", re.M)
_DECL = re.compile(r"^[ \t]*(int|int64_t)\s+(surf_\w+)\s*\(([^()]*)\)\s*;", re.M)
# `int` entry points whose result is a value (a count, a size, a yes/no), not a status: lib() gives them no errcheck
VALUE_RETURNING = frozenset({"surf_abi_version", "surf_blend_raw_floats", "surf_blend_packed_floats",
                             "surf_blend_backward_row_floats", "surf_spconv_wgrad_mfma_supported"})


def parse_header(text):
    """The text of a C header -> {name: (restype, argtypes)} of its `int|int64_t surf_*(...);` declarations.  A parameter type
    outside _CTYPES, or a declaration that only begins like one, raises with the function's name: nothing is guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    sigs = {}
    for res, name, params in _DECL.findall(text):
        args = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            ctype = ctypes.c_void_p if "*" in param else _CTYPES.get(" ".join(param.split()[:-1]))   # the type without the name
            if ctype is None:
                raise ValueError(f"{name}: no ctypes type for the parameter `{param.strip()}`")
            args.append(ctype)
        sigs[name] = (_CTYPES[res], args)
    partial = [name for name in _DECL_HEAD.findall(text) if name not in sigs]
    if partial:
        raise ValueError(f"{', '.join(partial)}: declaration not understood")
    return sigs


try:
    with open(HEADER_PATH) as _f:
        _header = _f.read()
except OSError as e:
    raise RuntimeError(f"{HEADER_PATH}: the C header the binding is derived from cannot be read ({e.strerror})") from None
# name -> (restype, argtypes), and the version lib() insists on: include/surf_hip.h is the only place either is written
SIGNATURES = parse_header(_header)
ABI_VERSION = int(re.search(r"^#define\s+SURF_ABI_VERSION\s+(\d+)", _header, re.M).group(1))

_lib = None


def build(verbose=False):
    """Compile the HIP sources for gfx950 (cross-compiles without a GPU)."""
    script = os.path.join(_HERE, "csrc", "build.sh")
    res = subprocess.run(["bash", script], capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode != 0:
        raise RuntimeError("building libsurf_hip.so failed")


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with surf_amd/csrc/build.sh (or __graft_entry__.build()). "
                "There is no CPU fallback for the SuRF hot path.")
        cand = ctypes.CDLL(LIB_PATH)
        rebuild = "rebuild with surf_amd/csrc/build.sh (or __graft_entry__.build())"
        try:                                  # the version first: a stale library lacks newer symbols and would otherwise
            cand.surf_abi_version.restype = ctypes.c_int         # die with a bare AttributeError in the binding loop below
            cand.surf_abi_version.argtypes = []
            got = cand.surf_abi_version()
        except AttributeError:
            raise RuntimeError(f"{LIB_PATH} exports no surf_abi_version: not a surf_hip library; {rebuild}") from None
        if got != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} reports ABI version {got}, include/surf_hip.h declares {ABI_VERSION}: {rebuild}")
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(cand, name)
            except AttributeError:
                raise RuntimeError(f"{LIB_PATH} (ABI {got}) lacks {name}, which include/surf_hip.h declares: {rebuild}") from None
            fn.restype = res
            fn.argtypes = args
            if res is ctypes.c_int and name not in VALUE_RETURNING:
                fn.errcheck = _raise_on_status
        _lib = cand                           # cached only when fully bound
    return _lib


class SurfHipError(RuntimeError):
    pass


def check(code, what):
    if code != 0:
        kind = {-1: "invalid argument", -2: "exceeds a SURF_MAX_* limit"}.get(code, f"hipError {code}")
        raise SurfHipError(f"{what}: {kind}")


def _raise_on_status(code, fn, args):
    """errcheck of the status-returning entry points: 0 passes through, anything else raises with the entry point's name and
    the scalar arguments of the call (sizes, strides, modes: what tells one launch of a kernel from another)."""
    if code != 0:
        scalars = ", ".join(repr(getattr(a, "value", a)) for t, a in zip(fn.argtypes, args) if t is not ctypes.c_void_p)
        check(code, f"{fn.__name__}({scalars})")
    return code
