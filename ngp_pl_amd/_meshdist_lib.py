"""ctypes binding of libngp_meshdist.so (C ABI: include/ngp_meshdist.h): surface samples of a mesh, the nearest face of a target
mesh for every query point, and the weighted distance statistics.

A table of its own, as the other mesh libraries and libngp_metrics.so have: their entry points do not change.  torch is imported
first (through `_lib`) so that the library binds to the HIP runtime torch already loaded.  No fallback: a missing library or a
failing call raises.
"""
import ctypes as C
import os

from ._lib import NgpError, device_guard, ptr, stream  # noqa: F401  (re-exported for mesh.py)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libngp_meshdist.so")
ABI_VERSION = 1

# mirrors of the header's constants (tests/test_meshdist_cpu.py holds them equal)
K_MAX, MAX_AXIS, MAX_CELLS, MAX_THRESHOLDS = 64, 1024, 1 << 30, 8
SLACK_ULPS, MIN_CELL_SLACKS = 64, 8
SCAN_BLOCK, STATS_MAX_BLOCKS, STATS_OUTPUTS = 2048, 512, 14

P, I, L, Z, F = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float
F3 = C.POINTER(C.c_float)

# name -> argtypes (every function returns int)
_PROTOS = {
    "ngp_meshdist_abi_version": [],
    "ngp_meshdist_slack": [F3, F, I, I, I, F3, F3],
    "ngp_meshdist_sample_count": [P, P, L, L, F, P, Z, P, P],
    "ngp_meshdist_sample_emit": [P, P, L, L, F, P, Z, L, P, P, P, P],
    "ngp_meshdist_grid_count": [P, P, L, L, F3, F, I, I, I, P, Z, P, P],
    "ngp_meshdist_grid_fill": [P, P, L, L, F3, F, I, I, I, P, Z, L, P, P],
    "ngp_meshdist_query": [P, L, P, P, L, L, F3, F, I, I, I, F, P, Z, P, L, P, P, P, P, P],
    "ngp_meshdist_stats": [P, P, P, L, F3, I, P, Z, P, P],
}
_SIZES = {
    "ngp_meshdist_sample_workspace_bytes": [L],
    "ngp_meshdist_grid_workspace_bytes": [I, I, I],
    "ngp_meshdist_stats_workspace_bytes": [L],
}
_ERRORS = {-1: "NGP_EINVAL (bad argument; for a grid also a cell below 2^-14 of the grid's largest coordinate magnitude)",
           -5: "NGP_ERANGE (more than INT32_MAX vertices, faces, samples, grid entries or points)"}

_h = None


def lib():
    global _h
    if _h is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libngp_meshdist.so is missing (%s): run `python -m ngp_pl_amd.build` or __graft_entry__.build(); "
                               "there is no CPU/eager fallback" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            f = getattr(h, name)
            f.argtypes = argtypes
            f.restype = I
        for name, argtypes in _SIZES.items():
            f = getattr(h, name)
            f.argtypes = argtypes
            f.restype = Z
        h.ngp_meshdist_build_arch.argtypes = []
        h.ngp_meshdist_build_arch.restype = C.c_char_p
        if h.ngp_meshdist_abi_version() != ABI_VERSION:
            raise RuntimeError("%s has ABI version %d, this package binds version %d: rebuild the library (python -m ngp_pl_amd.build)"
                               % (LIB_PATH, h.ngp_meshdist_abi_version(), ABI_VERSION))
        _h = h
    return _h


def exported_symbols():
    return list(_PROTOS) + list(_SIZES) + ["ngp_meshdist_build_arch"]


def floats(values):
    """A host float array for the `origin` and `thresholds` arguments."""
    values = [float(v) for v in values]
    return (C.c_float * max(len(values), 1))(*values)


def slack(origin, cell, dims):
    """(slack(M_grid), the smallest cell the grid accepts) as the library computes them in f32."""
    s, m = C.c_float(), C.c_float()
    call("ngp_meshdist_slack", floats(origin), cell, int(dims[0]), int(dims[1]), int(dims[2]), C.byref(s), C.byref(m))
    return s.value, m.value


def call(name, *args):
    """Invoke an entry point; a non-zero status raises _lib.NgpError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise NgpError("%s failed: %s" % (name, _ERRORS.get(rc, "hipError_t %d" % rc)))
    return 0
