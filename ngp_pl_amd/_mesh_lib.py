"""ctypes binding of libngp_mesh.so (C ABI: include/ngp_mesh.h), the mesh-export library.

Kept apart from `_lib.py`'s table: mesh export is not part of the drop-in boundary of libngp_hip.so.  torch is imported first (through
`_lib`) so that the library binds to the HIP runtime torch already loaded.  No fallback: a missing library or a failing call raises.
"""
import ctypes as C
import os

from . import _lib
from ._lib import NgpError, device_guard, ptr, stream  # noqa: F401  (re-exported for mesh.py)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libngp_mesh.so")
ABI_VERSION = 1

P, I, F, L = C.c_void_p, C.c_int, C.c_float, C.c_int64

# name -> argtypes (every function returns int)
_PROTOS = {
    "ngp_mesh_abi_version": [],
    "ngp_mesh_lattice_points": [I, I, I, P, L, L, P, P],
    "ngp_mesh_count": [P, I, I, I, F, P, C.c_size_t, P, P],
    "ngp_mesh_emit": [P, I, I, I, F, P, P, C.c_size_t, L, L, P, P, P, P],
}
_ERRORS = {-1: "NGP_EINVAL (bad argument)", -5: "NGP_ERANGE (more than INT32_MAX vertices or faces)"}

_h = None


def lib():
    global _h
    if _h is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libngp_mesh.so is missing (%s): run `python -m ngp_pl_amd.build` or __graft_entry__.build(); "
                               "there is no CPU/eager fallback" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            f = getattr(h, name)
            f.argtypes = argtypes
            f.restype = I
        h.ngp_mesh_build_arch.argtypes = []
        h.ngp_mesh_build_arch.restype = C.c_char_p
        h.ngp_mesh_workspace_bytes.argtypes = [I, I, I]
        h.ngp_mesh_workspace_bytes.restype = C.c_size_t
        if h.ngp_mesh_abi_version() != ABI_VERSION:
            raise RuntimeError("%s has ABI version %d, this package binds version %d: rebuild the library (python -m ngp_pl_amd.build)"
                               % (LIB_PATH, h.ngp_mesh_abi_version(), ABI_VERSION))
        _h = h
    return _h


def exported_symbols():
    return list(_PROTOS) + ["ngp_mesh_build_arch", "ngp_mesh_workspace_bytes"]


def call(name, *args):
    """Invoke an entry point; a non-zero status raises _lib.NgpError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise NgpError("%s failed: %s" % (name, _ERRORS.get(rc, "hipError_t %d" % rc)))
    return 0


def bounds6(lo, hi):
    """HOST float[6] {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z}."""
    return (C.c_float * 6)(*[float(v) for v in list(lo) + list(hi)])
