"""ctypes binding of libngp_meshchart.so (C ABI: csrc/meshchart/ngp_meshchart.h): the texture atlas made of charts (class per
face, the vertex table, chart labels, bounds, the host packer, texel owners, eviction, dilation, corners and UVs, texel points)
and its renderer.

A table of its own, as the other mesh libraries have: their entry points do not change.  torch is imported first (through `_lib`)
so that the library binds to the HIP runtime torch already loaded.  No fallback: a missing library or a failing call raises.
"""
import ctypes as C
import os

import numpy as np

from ._lib import NgpError, device_guard, ptr, stream  # noqa: F401  (re-exported for mesh.py)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libngp_meshchart.so")
ABI_VERSION = 1
NO_CLASS = 6
MAX_PAD = 8

P, I, L, Z, F = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float

# name -> argtypes (every function returns int)
_PROTOS = {
    "ngp_meshchart_abi_version": [],
    "ngp_meshchart_classify": [P, P, L, L, F, P, P, P, P, Z, P],
    "ngp_meshchart_label": [P, L, L, P, P, P, P, I, L, P, P, P, P, Z, P],
    "ngp_meshchart_bounds": [P, P, L, L, F, P, L, L, P, P],
    "ngp_meshchart_pack": [P, L, I, I, I, P, P, P, P],
    "ngp_meshchart_raster": [P, P, L, L, F, P, P, L, L, L, I, I, I, P, P],
    "ngp_meshchart_evict": [P, P, L, L, F, P, P, L, L, L, I, I, I, P, P, P, P],
    "ngp_meshchart_dilate": [P, P, I, I, I, P],
    "ngp_meshchart_corners": [P, P, L, L, F, P, P, L, I, I, I, P, P, P],
    "ngp_meshchart_texel_points": [P, P, P, L, L, P, I, I, P, P, L, L, P, P, P, P],
    "ngp_meshchart_render": [P, P, L, L, P, P, I, I, P, P, L, I, I, F, P, P, Z, P, P, P, P],
}
_ERRORS = {-1: "NGP_EINVAL (bad argument)",
           -5: "NGP_ERANGE (more than INT32_MAX vertices, faces or cameras, or an atlas wider or higher than 16384 texels)"}

_h = None


def lib():
    global _h
    if _h is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libngp_meshchart.so is missing (%s): run `python -m ngp_pl_amd.build` or __graft_entry__.build(); "
                               "there is no CPU/eager fallback" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            f = getattr(h, name)
            f.argtypes = argtypes
            f.restype = I
        h.ngp_meshchart_build_arch.argtypes = []
        h.ngp_meshchart_build_arch.restype = C.c_char_p
        h.ngp_meshchart_classify_workspace_bytes.argtypes = [L, L]
        h.ngp_meshchart_classify_workspace_bytes.restype = Z
        h.ngp_meshchart_label_workspace_bytes.argtypes = [L]
        h.ngp_meshchart_label_workspace_bytes.restype = Z
        h.ngp_meshchart_render_workspace_bytes.argtypes = [I, I, L]
        h.ngp_meshchart_render_workspace_bytes.restype = Z
        if h.ngp_meshchart_abi_version() != ABI_VERSION:
            raise RuntimeError("%s has ABI version %d, this package binds version %d: rebuild the library (python -m ngp_pl_amd.build)"
                               % (LIB_PATH, h.ngp_meshchart_abi_version(), ABI_VERSION))
        _h = h
    return _h


def exported_symbols():
    return list(_PROTOS) + ["ngp_meshchart_build_arch", "ngp_meshchart_classify_workspace_bytes", "ngp_meshchart_label_workspace_bytes",
                            "ngp_meshchart_render_workspace_bytes"]


def call(name, *args):
    """Invoke an entry point; a non-zero status raises _lib.NgpError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise NgpError("%s failed: %s" % (name, _ERRORS.get(rc, "hipError_t %d" % rc)))
    return 0


def pack(sizes, sort=True, width=0, y0=0):
    """ngp_meshchart_pack of the (n, 2) rectangle sizes (w, h) -> (origins (n, 2) int32 array, order (n,) int32 array, W, H so far);
    ValueError when the atlas does not fit 16384 texels.  Host only."""
    sizes = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))
    n = len(sizes)
    origins, order = np.empty((n, 2), np.int32), np.empty(n, np.int32)
    w, h = I(), I()
    rc = lib().ngp_meshchart_pack(sizes.ctypes.data, n, int(bool(sort)), int(width), int(y0), origins.ctypes.data, order.ctypes.data,
                                  C.byref(w), C.byref(h))
    if rc == -5:
        raise ValueError("the atlas of %d charts is wider or higher than 16384 texels: raise texel_size or simplify the mesh" % n)
    if rc:
        raise NgpError("ngp_meshchart_pack failed: %s" % _ERRORS.get(rc, rc))
    return origins, order, w.value, h.value
