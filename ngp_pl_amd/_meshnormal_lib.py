"""ctypes binding of libngp_meshnormal.so (C ABI: csrc/meshnormal/ngp_meshnormal.h): the normals of a detail mesh carried onto
query points through the nearest face that faces the same way (exactly the brute-force minimum, through the grid of
libngp_meshdist.so), and the shading of a rendered frame by a rendered normal map.

A table of its own, as the other mesh libraries have: their entry points do not change.  torch is imported first (through `_lib`)
so that the library binds to the HIP runtime torch already loaded.  No fallback: a missing library or a failing call raises.
"""
import ctypes as C
import os

from ._lib import NgpError, device_guard, ptr, stream  # noqa: F401  (re-exported for mesh.py)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libngp_meshnormal.so")
ABI_VERSION = 1

# mirrors of the header's constants (tests/test_meshnormal_cpu.py holds them equal, and equal to libngp_meshdist.so's)
MAX_SHELLS = 8
MAX_AXIS, MAX_CELLS = 1024, 1 << 30
SLACK_ULPS, MIN_CELL_SLACKS, SCAN_BLOCK = 64, 8, 2048

P, I, L, Z, F = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float
F3 = C.POINTER(C.c_float)

# name -> argtypes (every function returns int)
_PROTOS = {
    "ngp_meshnormal_abi_version": [],
    "ngp_meshnormal_transfer": [P, P, P, L, P, P, P, L, L, F3, F, I, I, I, P, Z, P, L, F, I, P, P, P, P, P, P],
    "ngp_meshnormal_shade": [P, P, P, P, L, I, I, F, P, P],
}
_ERRORS = {-1: "NGP_EINVAL (bad argument; for a transfer also a max_dist that is not finite or is above %d cells of the grid)" % MAX_SHELLS,
           -5: "NGP_ERANGE (more than INT32_MAX queries, vertices, faces, grid entries or pixels in one call)"}

_h = None


def lib():
    global _h
    if _h is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libngp_meshnormal.so is missing (%s): run `python -m ngp_pl_amd.build` or __graft_entry__.build(); "
                               "there is no CPU/eager fallback" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            f = getattr(h, name)
            f.argtypes = argtypes
            f.restype = I
        h.ngp_meshnormal_build_arch.argtypes = []
        h.ngp_meshnormal_build_arch.restype = C.c_char_p
        if h.ngp_meshnormal_abi_version() != ABI_VERSION:
            raise RuntimeError("%s has ABI version %d, this package binds version %d: rebuild the library (python -m ngp_pl_amd.build)"
                               % (LIB_PATH, h.ngp_meshnormal_abi_version(), ABI_VERSION))
        _h = h
    return _h


def exported_symbols():
    return list(_PROTOS) + ["ngp_meshnormal_build_arch"]


def floats(values):
    """A host float array for the `origin` argument."""
    values = [float(v) for v in values]
    return (C.c_float * max(len(values), 1))(*values)


def call(name, *args):
    """Invoke an entry point; a non-zero status raises _lib.NgpError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise NgpError("%s failed: %s" % (name, _ERRORS.get(rc, "hipError_t %d" % rc)))
    return 0
