"""ctypes binding of libngp_meshatlas.so (C ABI: csrc/meshatlas/ngp_meshatlas.h): the texture atlas with texel density by face size
(class per face, the stable sort by class, the banded layout, texel points and directions, UVs) and its renderer.

A table of its own, as the other mesh libraries have: their entry points do not change.  torch is imported first (through `_lib`)
so that the library binds to the HIP runtime torch already loaded.  No fallback: a missing library or a failing call raises.
"""
import ctypes as C
import os

from ._lib import NgpError, device_guard, ptr, stream  # noqa: F401  (re-exported for mesh.py)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libngp_meshatlas.so")
ABI_VERSION = 1
CLASSES = 16
LADDER = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256)          # T_c of the header's ladder

P, I, L, Z, F = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float

# name -> argtypes (every function returns int)
_PROTOS = {
    "ngp_meshatlas_abi_version": [],
    "ngp_meshatlas_classify": [P, P, L, L, F, I, I, P, P, P, P, Z, P],
    "ngp_meshatlas_layout": [P, P, P, P],
    "ngp_meshatlas_place": [P, P, L, P, P],
    "ngp_meshatlas_texel_points": [P, P, P, L, L, P, P, P, L, L, P, P, P, P],
    "ngp_meshatlas_face_uvs": [P, L, I, I, P, P],
    "ngp_meshatlas_render": [P, P, L, L, P, P, I, I, P, P, L, I, I, F, P, P, Z, P, P, P, P],
}
_ERRORS = {-1: "NGP_EINVAL (bad argument)",
           -5: "NGP_ERANGE (more than INT32_MAX vertices, faces or cameras, or an atlas wider or higher than 16384 texels)"}

_h = None


def lib():
    global _h
    if _h is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libngp_meshatlas.so is missing (%s): run `python -m ngp_pl_amd.build` or __graft_entry__.build(); "
                               "there is no CPU/eager fallback" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            f = getattr(h, name)
            f.argtypes = argtypes
            f.restype = I
        h.ngp_meshatlas_build_arch.argtypes = []
        h.ngp_meshatlas_build_arch.restype = C.c_char_p
        h.ngp_meshatlas_classify_workspace_bytes.argtypes = [L]
        h.ngp_meshatlas_classify_workspace_bytes.restype = Z
        h.ngp_meshatlas_render_workspace_bytes.argtypes = [I, I, L]
        h.ngp_meshatlas_render_workspace_bytes.restype = Z
        if h.ngp_meshatlas_abi_version() != ABI_VERSION:
            raise RuntimeError("%s has ABI version %d, this package binds version %d: rebuild the library (python -m ngp_pl_amd.build)"
                               % (LIB_PATH, h.ngp_meshatlas_abi_version(), ABI_VERSION))
        _h = h
    return _h


def exported_symbols():
    return list(_PROTOS) + ["ngp_meshatlas_build_arch", "ngp_meshatlas_classify_workspace_bytes", "ngp_meshatlas_render_workspace_bytes"]


def call(name, *args):
    """Invoke an entry point; a non-zero status raises _lib.NgpError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise NgpError("%s failed: %s" % (name, _ERRORS.get(rc, "hipError_t %d" % rc)))
    return 0


def layout(counts):
    """ngp_meshatlas_layout of 16 host counts -> (width, height, bands as 16 tuples (y, h, cells_per_row, cells)); ValueError when
    the atlas does not fit 16384 texels."""
    arr = (L * CLASSES)(*[int(c) for c in counts])
    w, h = I(), I()
    bands = (C.c_int32 * (4 * CLASSES))()
    rc = lib().ngp_meshatlas_layout(arr, C.byref(w), C.byref(h), bands)
    if rc == -5:
        raise ValueError("the atlas of the class counts %r is wider than 16384 texels: raise texel_size, lower max_texels or simplify the mesh"
                         % (list(arr),))
    if rc:
        raise NgpError("ngp_meshatlas_layout failed: %s" % _ERRORS.get(rc, rc))
    return w.value, h.value, [tuple(bands[4 * c:4 * c + 4]) for c in range(CLASSES)]
