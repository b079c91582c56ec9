"""ctypes binding of libngp_meshsparse.so (C ABI: csrc/meshsparse/ngp_meshsparse.h): marching cubes over the bricks of the lattice
that touch occupied cells (the mask from the occupancy bitfield, dilation and slot lists, the points of the sampled bricks, count and
emit).

A table of its own, as the other mesh libraries have: their entry points do not change.  torch is imported first (through `_lib`)
so that the library binds to the HIP runtime torch already loaded.  No fallback: a missing library or a failing call raises.
"""
import ctypes as C
import os

from ._lib import NgpError, device_guard, ptr, stream  # noqa: F401  (re-exported for mesh.py)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libngp_meshsparse.so")
ABI_VERSION = 1
BRICK = 8
BRICK_POINTS = 512

P, I, L, Z, F, D = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float, C.c_double

# name -> argtypes (every function returns int)
_PROTOS = {
    "ngp_meshsparse_abi_version": [],
    "ngp_meshsparse_mask": [P, I, I, F, I, I, I, P, D, P, P],
    "ngp_meshsparse_index_count": [P, I, I, I, P, Z, P, P],
    "ngp_meshsparse_index_fill": [P, I, I, I, P, Z, L, L, P, P, P, P],
    "ngp_meshsparse_points": [I, I, I, P, P, L, L, L, P, P],
    "ngp_meshsparse_count": [P, I, I, I, F, P, P, P, L, P, L, P, Z, P, P],
    "ngp_meshsparse_emit": [P, I, I, I, F, P, P, P, L, P, L, P, Z, L, L, P, P, P, P, P, P],
}
_ERRORS = {-1: "NGP_EINVAL (bad argument)", -5: "NGP_ERANGE (more than INT32_MAX vertices or faces)"}

_h = None


def lib():
    global _h
    if _h is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libngp_meshsparse.so is missing (%s): run `python -m ngp_pl_amd.build` or __graft_entry__.build(); "
                               "there is no CPU/eager fallback" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            f = getattr(h, name)
            f.argtypes = argtypes
            f.restype = I
        h.ngp_meshsparse_build_arch.argtypes = []
        h.ngp_meshsparse_build_arch.restype = C.c_char_p
        h.ngp_meshsparse_index_workspace_bytes.argtypes = [I, I, I]
        h.ngp_meshsparse_index_workspace_bytes.restype = Z
        h.ngp_meshsparse_workspace_bytes.argtypes = [L, L]
        h.ngp_meshsparse_workspace_bytes.restype = Z
        if h.ngp_meshsparse_abi_version() != ABI_VERSION:
            raise RuntimeError("%s has ABI version %d, this package binds version %d: rebuild the library (python -m ngp_pl_amd.build)"
                               % (LIB_PATH, h.ngp_meshsparse_abi_version(), ABI_VERSION))
        _h = h
    return _h


def exported_symbols():
    return list(_PROTOS) + ["ngp_meshsparse_build_arch", "ngp_meshsparse_index_workspace_bytes", "ngp_meshsparse_workspace_bytes"]


def call(name, *args):
    """Invoke an entry point; a non-zero status raises _lib.NgpError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise NgpError("%s failed: %s" % (name, _ERRORS.get(rc, "hipError_t %d" % rc)))
    return 0
