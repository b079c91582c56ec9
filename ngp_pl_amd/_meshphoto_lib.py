"""ctypes binding of libngp_meshphoto.so (C ABI: csrc/meshphoto/ngp_meshphoto.h): the colour of surface points blended from
photographs with known cameras (projection, the two-sided depth test against the mesh's depth buffers, the bilinear sample, the
weight by viewing angle, the serial per-point sums) and the resolve of the sums into colours.

A table of its own, as the other mesh libraries have: their entry points do not change.  torch is imported first (through `_lib`)
so that the library binds to the HIP runtime torch already loaded.  No fallback: a missing library or a failing call raises.
"""
import ctypes as C
import os

from ._lib import NgpError, device_guard, ptr, stream  # noqa: F401  (re-exported for mesh.py)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libngp_meshphoto.so")
ABI_VERSION = 1
CAM_TILE = 64                                           # cameras per LDS tile of photo_accumulate (csrc/meshphoto/meshphoto.hip)
MAX_GUARD = 4
MAX_POWER = 8

P, I, L, F = C.c_void_p, C.c_int, C.c_int64, C.c_float

# name -> argtypes (every function returns int)
_PROTOS = {
    "ngp_meshphoto_abi_version": [],
    "ngp_meshphoto_accumulate": [P, P, P, L, P, P, L, I, I, P, P, F, F, I, F, I, P, P, P],
    "ngp_meshphoto_resolve": [P, P, P, L, C.c_int32, P, P, P],
}
_ERRORS = {-1: "NGP_EINVAL (bad argument)",
           -5: "NGP_ERANGE (more than INT32_MAX points or cameras in one call)"}

_h = None


def lib():
    global _h
    if _h is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libngp_meshphoto.so is missing (%s): run `python -m ngp_pl_amd.build` or __graft_entry__.build(); "
                               "there is no CPU/eager fallback" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            f = getattr(h, name)
            f.argtypes = argtypes
            f.restype = I
        h.ngp_meshphoto_build_arch.argtypes = []
        h.ngp_meshphoto_build_arch.restype = C.c_char_p
        if h.ngp_meshphoto_abi_version() != ABI_VERSION:
            raise RuntimeError("%s has ABI version %d, this package binds version %d: rebuild the library (python -m ngp_pl_amd.build)"
                               % (LIB_PATH, h.ngp_meshphoto_abi_version(), ABI_VERSION))
        _h = h
    return _h


def exported_symbols():
    return list(_PROTOS) + ["ngp_meshphoto_build_arch"]


def call(name, *args):
    """Invoke an entry point; a non-zero status raises _lib.NgpError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise NgpError("%s failed: %s" % (name, _ERRORS.get(rc, "hipError_t %d" % rc)))
    return 0
