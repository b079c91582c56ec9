"""ctypes binding of libngp_meshdecimate.so (C ABI: include/ngp_meshdecimate.h): decimation of a mesh by rounds of independent
half-edge collapses.

A table of its own, as `_meshsimplify_lib.py` and the other mesh bindings have: the entry points of the other libraries do not
change.  torch is imported first (through `_lib`) so that the library binds to the HIP runtime torch already loaded.  No fallback:
a missing library or a failing call raises.
"""
import ctypes as C
import os

from ._lib import NgpError, device_guard, ptr, stream  # noqa: F401  (re-exported for mesh.py)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libngp_meshdecimate.so")
ABI_VERSION = 1
MAX_DEGREE = 64                          # a vertex with more corners is never removed
MAX_FACES = (2 ** 31 - 1) // 3           # a corner's number fits int32

P, I, L, Z, F = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float

# name -> argtypes (every function returns int)
_PROTOS = {
    "ngp_meshdecimate_abi_version": [],
    "ngp_meshdecimate_begin": [P, L, L, P, Z, P],
    "ngp_meshdecimate_round": [P, L, L, F, F, P, Z, P, P],
    "ngp_meshdecimate_apply": [L, L, L, L, P, Z, P],
    "ngp_meshdecimate_count": [L, L, P, Z, P, P],
    "ngp_meshdecimate_emit": [P, P, P, L, L, P, Z, L, L, P, P, P, P, P],
}
_ERRORS = {-1: "NGP_EINVAL (bad argument)", -5: "NGP_ERANGE (more than INT32_MAX vertices or INT32_MAX / 3 faces)"}

_h = None


def lib():
    global _h
    if _h is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libngp_meshdecimate.so is missing (%s): run `python -m ngp_pl_amd.build` or __graft_entry__.build(); "
                               "there is no CPU/eager fallback" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            f = getattr(h, name)
            f.argtypes = argtypes
            f.restype = I
        h.ngp_meshdecimate_build_arch.argtypes = []
        h.ngp_meshdecimate_build_arch.restype = C.c_char_p
        h.ngp_meshdecimate_workspace_bytes.argtypes = [L, L]
        h.ngp_meshdecimate_workspace_bytes.restype = Z
        if h.ngp_meshdecimate_abi_version() != ABI_VERSION:
            raise RuntimeError("%s has ABI version %d, this package binds version %d: rebuild the library (python -m ngp_pl_amd.build)"
                               % (LIB_PATH, h.ngp_meshdecimate_abi_version(), ABI_VERSION))
        _h = h
    return _h


def exported_symbols():
    return list(_PROTOS) + ["ngp_meshdecimate_build_arch", "ngp_meshdecimate_workspace_bytes"]


def call(name, *args):
    """Invoke an entry point; a non-zero status raises _lib.NgpError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise NgpError("%s failed: %s" % (name, _ERRORS.get(rc, "hipError_t %d" % rc)))
    return 0
