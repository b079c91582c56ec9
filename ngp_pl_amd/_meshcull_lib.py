"""ctypes binding of libngp_meshcull.so (C ABI: include/ngp_meshcull.h): depth-buffer visibility of a mesh against cameras and the
cull of the faces no camera sees.

A table of its own, as `_mesh_lib.py` and `_meshfilter_lib.py` have: the entry points of the other three libraries do not change.  torch is imported first (through `_lib`) so that the library binds to the HIP runtime torch already loaded.  No fallback:
a missing library or a failing call raises.
"""
import ctypes as C
import os

from ._lib import NgpError, device_guard, ptr, stream  # noqa: F401  (re-exported for mesh.py)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libngp_meshcull.so")
ABI_VERSION = 1

P, I, L, Z, F = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float

# name -> argtypes (every function returns int)
_PROTOS = {
    "ngp_meshcull_abi_version": [],
    "ngp_meshcull_views": [P, P, L, L, P, P, L, I, I, F, F, P, Z, P, P],
    "ngp_meshcull_count": [P, P, I, L, L, P, Z, P, P],
    "ngp_meshcull_emit": [P, P, I, P, P, P, L, L, P, Z, L, L, P, P, P, P, P],
}
_ERRORS = {-1: "NGP_EINVAL (bad argument)", -5: "NGP_ERANGE (more than INT32_MAX vertices, faces or cameras)"}

_h = None


def lib():
    global _h
    if _h is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libngp_meshcull.so is missing (%s): run `python -m ngp_pl_amd.build` or __graft_entry__.build(); "
                               "there is no CPU/eager fallback" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            f = getattr(h, name)
            f.argtypes = argtypes
            f.restype = I
        h.ngp_meshcull_build_arch.argtypes = []
        h.ngp_meshcull_build_arch.restype = C.c_char_p
        h.ngp_meshcull_workspace_bytes.argtypes = [L, L]
        h.ngp_meshcull_workspace_bytes.restype = Z
        h.ngp_meshcull_zbuffer_bytes.argtypes = [I, I, L]
        h.ngp_meshcull_zbuffer_bytes.restype = Z
        if h.ngp_meshcull_abi_version() != ABI_VERSION:
            raise RuntimeError("%s has ABI version %d, this package binds version %d: rebuild the library (python -m ngp_pl_amd.build)"
                               % (LIB_PATH, h.ngp_meshcull_abi_version(), ABI_VERSION))
        _h = h
    return _h


def exported_symbols():
    return list(_PROTOS) + ["ngp_meshcull_build_arch", "ngp_meshcull_workspace_bytes", "ngp_meshcull_zbuffer_bytes"]


def call(name, *args):
    """Invoke an entry point; a non-zero status raises _lib.NgpError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise NgpError("%s failed: %s" % (name, _ERRORS.get(rc, "hipError_t %d" % rc)))
    return 0
