"""ctypes binding of libngp_meshtex.so (C ABI: include/ngp_meshtex.h): the texture atlas of a mesh (layout, texel points and
directions, UVs) and the renderer of the textured mesh.

A table of its own, as the other mesh libraries have: their entry points do not change.  torch is imported first (through `_lib`)
so that the library binds to the HIP runtime torch already loaded.  No fallback: a missing library or a failing call raises.
"""
import ctypes as C
import os

from ._lib import NgpError, device_guard, ptr, stream  # noqa: F401  (re-exported for mesh.py)

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libngp_meshtex.so")
ABI_VERSION = 1

P, I, L, Z, F = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float

# name -> argtypes (every function returns int)
_PROTOS = {
    "ngp_meshtex_abi_version": [],
    "ngp_meshtex_atlas_size": [L, I, P, P, P],
    "ngp_meshtex_texel_points": [P, P, P, L, L, I, P, L, L, P, P, P, P],
    "ngp_meshtex_face_uvs": [L, I, P, P],
    "ngp_meshtex_render": [P, P, L, L, I, P, P, P, L, I, I, F, P, P, Z, P, P, P, P],
}
_ERRORS = {-1: "NGP_EINVAL (bad argument)",
           -5: "NGP_ERANGE (more than INT32_MAX vertices, faces or cameras, or an atlas wider or higher than 16384 texels)"}

_h = None


def lib():
    global _h
    if _h is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libngp_meshtex.so is missing (%s): run `python -m ngp_pl_amd.build` or __graft_entry__.build(); "
                               "there is no CPU/eager fallback" % LIB_PATH)
        h = C.CDLL(LIB_PATH)
        for name, argtypes in _PROTOS.items():
            f = getattr(h, name)
            f.argtypes = argtypes
            f.restype = I
        h.ngp_meshtex_build_arch.argtypes = []
        h.ngp_meshtex_build_arch.restype = C.c_char_p
        h.ngp_meshtex_render_workspace_bytes.argtypes = [I, I, L]
        h.ngp_meshtex_render_workspace_bytes.restype = Z
        if h.ngp_meshtex_abi_version() != ABI_VERSION:
            raise RuntimeError("%s has ABI version %d, this package binds version %d: rebuild the library (python -m ngp_pl_amd.build)"
                               % (LIB_PATH, h.ngp_meshtex_abi_version(), ABI_VERSION))
        _h = h
    return _h


def exported_symbols():
    return list(_PROTOS) + ["ngp_meshtex_build_arch", "ngp_meshtex_render_workspace_bytes"]


def call(name, *args):
    """Invoke an entry point; a non-zero status raises _lib.NgpError."""
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise NgpError("%s failed: %s" % (name, _ERRORS.get(rc, "hipError_t %d" % rc)))
    return 0
