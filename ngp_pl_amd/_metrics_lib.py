"""ctypes binding of libngp_metrics.so (C ABI: include/ngp_metrics.h): the squared error behind PSNR and SSIM with the Gaussian
window, per image of a batch.

A table of its own, as the mesh libraries have: their entry points do not change.  torch is imported first (through `_lib`)
so that the library binds to the HIP runtime torch already loaded.  No fallback: a missing library or a failing call raises.
"""
import ctypes as C
import os

from ._lib import NgpError, device_guard, ptr, stream  # noqa: F401  (re-exported for metrics.py)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libngp_metrics.so")
ABI_VERSION = 1

# mirrors of the header's constants (tests/test_metrics_cpu.py holds them equal)
HWC, CHW = 0, 1
TILE_W, TILE_H = 64, 12
SQ_THREADS, SQ_MAX_BLOCKS = 256, 512
MAX_CHANNELS, MAX_SIDE, WINDOW_TAPS = 4, 16384, 11

P, I, L, Z, D = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_double

# name -> argtypes (every function returns int)
_PROTOS = {
    "ngp_metrics_abi_version": [],
    "ngp_metrics_tile": [C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "ngp_metrics_sq_error": [P, P, P, L, I, I, I, I, P, Z, P, P, P],
    "ngp_metrics_ssim": [P, P, P, L, I, I, I, I, D, P, Z, P, P, P, P],
}
_ERRORS = {-1: "NGP_EINVAL (bad argument)",
           -5: "NGP_ERANGE (an image wider or higher than 16384 pixels, or more than INT32_MAX workgroup partials)"}

_h = None


def lib():
    global _h
    if _h is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libngp_metrics.so is missing (%s): run `python -m ngp_pl_amd.build` or __graft_entry__.build(); "
                               "there is no CPU/eager fallback" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            f = getattr(h, name)
            f.argtypes = argtypes
            f.restype = I
        h.ngp_metrics_build_arch.argtypes = []
        h.ngp_metrics_build_arch.restype = C.c_char_p
        h.ngp_metrics_workspace_bytes.argtypes = [L, I, I, I]
        h.ngp_metrics_workspace_bytes.restype = Z
        if h.ngp_metrics_abi_version() != ABI_VERSION:
            raise RuntimeError("%s has ABI version %d, this package binds version %d: rebuild the library (python -m ngp_pl_amd.build)"
                               % (LIB_PATH, h.ngp_metrics_abi_version(), ABI_VERSION))
        _h = h
    return _h


def exported_symbols():
    return list(_PROTOS) + ["ngp_metrics_build_arch", "ngp_metrics_workspace_bytes"]


def call(name, *args):
    """Invoke an entry point; a non-zero status raises _lib.NgpError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise NgpError("%s failed: %s" % (name, _ERRORS.get(rc, "hipError_t %d" % rc)))
    return 0
