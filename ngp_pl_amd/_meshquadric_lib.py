"""ctypes binding of libngp_meshquadric.so (C ABI: include/ngp_meshquadric.h): quadric placement of the vertices of a vertex
clustering.

A table of its own, as `_meshsimplify_lib.py` and the other mesh bindings have: the entry points of the other libraries do not
change.  torch is imported first (through `_lib`) so that the library binds to the HIP runtime torch already loaded.  No fallback:
a missing library or a failing call raises.
"""
import ctypes as C
import os

from ._lib import NgpError, device_guard, ptr, stream  # noqa: F401  (re-exported for mesh.py)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libngp_meshquadric.so")
ABI_VERSION = 1
SUMS = 14                                # int64 sums per cluster: n, P[3], A[6], B[3], Wsum
NOT_LEADER, QUADRIC, MEAN_NO_FACES, MEAN_OUTSIDE = 0, 1, 2, 3       # the values of `state`

P, I, L, Z, F = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float

# name -> argtypes (every function returns int)
_PROTOS = {
    "ngp_meshquadric_abi_version": [],
    "ngp_meshquadric_accumulate": [P, P, P, L, L, P, F, P, Z, P],
    "ngp_meshquadric_sums": [P, L, P, Z, P, P],
    "ngp_meshquadric_place": [P, P, L, P, F, P, Z, P, P, P, P],
}
_ERRORS = {-1: "NGP_EINVAL (bad argument)", -5: "NGP_ERANGE (more than INT32_MAX vertices or faces)"}

_h = None


def lib():
    global _h
    if _h is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libngp_meshquadric.so is missing (%s): run `python -m ngp_pl_amd.build` or __graft_entry__.build(); "
                               "there is no CPU/eager fallback" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            f = getattr(h, name)
            f.argtypes = argtypes
            f.restype = I
        h.ngp_meshquadric_build_arch.argtypes = []
        h.ngp_meshquadric_build_arch.restype = C.c_char_p
        h.ngp_meshquadric_workspace_bytes.argtypes = [L, L]
        h.ngp_meshquadric_workspace_bytes.restype = Z
        if h.ngp_meshquadric_abi_version() != ABI_VERSION:
            raise RuntimeError("%s has ABI version %d, this package binds version %d: rebuild the library (python -m ngp_pl_amd.build)"
                               % (LIB_PATH, h.ngp_meshquadric_abi_version(), ABI_VERSION))
        _h = h
    return _h


def exported_symbols():
    return list(_PROTOS) + ["ngp_meshquadric_build_arch", "ngp_meshquadric_workspace_bytes"]


def call(name, *args):
    """Invoke an entry point; a non-zero status raises _lib.NgpError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise NgpError("%s failed: %s" % (name, _ERRORS.get(rc, "hipError_t %d" % rc)))
    return 0
