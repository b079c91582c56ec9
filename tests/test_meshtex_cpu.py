"""CPU: the C ABI of libngp_meshtex.so (header, exports, ctypes, code object, the host-only atlas layout, host-side argument
checks), the Python API's argument checks, the CLI, the OBJ / MTL / PNG writer, and the numpy restatement the GPU tests compare
against (tests/mesh_texture_reference.py): a two-face atlas listed by hand, the tiling property of the bilinear footprint, and a
linear colour field baked and rendered within half a quantisation step."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import mesh_texture_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngp_meshtex.h")
OTHERS = ("ngp_hip.h", "ngp_mesh.h", "ngp_meshfilter.h", "ngp_meshcull.h", "ngp_meshsimplify.h", "ngp_meshtsdf.h", "ngp_meshsmooth.h")
F = np.float32


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


# ---- 1. the C ABI


def test_header_compiles_as_c99_alone_and_with_the_other_seven_in_several_orders():
    inc = lambda names: "".join('#include "%s"\n' % n for n in names)
    for src in ('#include "ngp_meshtex.h"\nint main(void) { return 0; }\n',
                inc(OTHERS + ("ngp_meshtex.h",)) + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n",
                inc(("ngp_meshtex.h",) + OTHERS[::-1]) + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n",
                inc(OTHERS[3:] + ("ngp_meshtex.h",) + OTHERS[:3]) + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n"):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}
    assert "#ifndef NGP_EINVAL" in text and "#ifndef NGP_ERANGE" in text and "THE RULE" in text


def test_library_exports_exactly_its_header():
    from ngp_pl_amd import _abi, _meshtex_lib
    protos = _abi.parse(HEADER)
    assert set(protos) == {"ngp_meshtex_" + n for n in ("abi_version", "build_arch", "atlas_size", "texel_points", "face_uvs",
                                                        "render_workspace_bytes", "render")}
    assert _exports(_meshtex_lib.LIB_PATH) == set(protos)
    assert set(_meshtex_lib.exported_symbols()) == set(protos)
    lib = _meshtex_lib.lib()
    assert lib.ngp_meshtex_abi_version() == 1 == _meshtex_lib.ABI_VERSION and lib.ngp_meshtex_build_arch() == b"gfx950"


def test_the_eight_libraries_share_no_symbol():
    from ngp_pl_amd import (_abi, _lib, _mesh_lib, _meshcull_lib, _meshfilter_lib, _meshsimplify_lib, _meshsmooth_lib, _meshtex_lib,
                            _meshtsdf_lib)
    mods = (_lib, _mesh_lib, _meshfilter_lib, _meshcull_lib, _meshsimplify_lib, _meshtsdf_lib, _meshsmooth_lib, _meshtex_lib)
    for m in mods:
        m.lib()
    assert len({m.LIB_PATH for m in mods}) == 8
    exports = [_exports(m.LIB_PATH) for m in mods]
    assert all(exports) and len(exports[0]) >= 100
    for i, a in enumerate(exports):
        for b in exports[i + 1:]:
            assert not a & b
    own, others = exports[-1], set().union(*exports[:-1])
    assert not [s for s in others if s.startswith("ngp_meshtex")]
    assert not [s for s in own if not s.startswith("ngp_meshtex_")]
    declared_elsewhere = set(_abi.parse_all())
    for h in OTHERS[1:]:
        declared_elsewhere |= set(_abi.parse(os.path.join(ROOT, "include", h)))
    assert not set(_abi.parse(HEADER)) & declared_elsewhere


def test_ctypes_agrees_with_the_header():
    from ngp_pl_amd import _abi, _meshtex_lib
    protos = _abi.parse(HEADER)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _meshtex_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    lib = _meshtex_lib.lib()
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        want = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret]
        assert f.restype is want, name


def test_code_object_is_gfx950_only():
    from ngp_pl_amd import _meshtex_lib
    blob = open(_meshtex_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob
    for kernel in (b"tex_points", b"tex_uvs", b"tex_raster", b"tex_shade"):
        assert kernel in blob


def test_build_links_the_eighth_library_with_contraction_off():
    from ngp_pl_amd import _meshtex_lib, build
    assert build.MESHTEX_LIB == _meshtex_lib.LIB_PATH and build.MESHTEX_CFLAGS == ["-ffp-contract=off"]
    assert build.ARCH == "gfx950" and all(os.path.exists(os.path.join(build.CSRC, s)) for s in build.MESHTEX_SOURCES)
    assert build.MESHTEX_SOURCES == [os.path.join("meshtex", "meshtex.hip")]


# ---- 2. the atlas layout against known answers


def _atlas(n_faces, T):
    from ngp_pl_amd import _meshtex_lib
    c, w, h = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    rc = _meshtex_lib.lib().ngp_meshtex_atlas_size(n_faces, T, C.byref(c), C.byref(w), C.byref(h))
    return rc, (c.value, w.value, h.value)


def test_atlas_size_known_answers():
    for n_faces, want in ((1, (1, 6, 5)), (2, (1, 6, 5)), (3, (2, 12, 5)), (4, (2, 12, 5)), (5, (2, 12, 10)), (6, (2, 12, 10))):
        assert _atlas(n_faces, 1) == (0, want) and TR.atlas_size(n_faces, 1) == want
    # T = 8: cells of 13 x 12; 100 cells: 10 per row give 130 x 120, 9 per row 117 < 12 * 12
    assert _atlas(200, 8) == (0, (10, 130, 120)) == (0, TR.atlas_size(200, 8))
    for n_faces in (1, 2, 7, 100, 1001, 65536, 659498):
        for T in (1, 2, 3, 8, 31, 256):
            try:
                want = TR.atlas_size(n_faces, T)
            except OverflowError:
                assert _atlas(n_faces, T) == (-5, (-7, -7, -7))
                continue
            rc, got = _atlas(n_faces, T)
            assert rc == 0 and got == want
            c, w, h = got
            cells = (n_faces + 1) // 2
            assert w == c * (T + 5) and h == -(-cells // c) * (T + 4) and w >= h and max(w, h) <= 16384
            assert c == 1 or (c - 1) * (T + 5) < -(-cells // (c - 1)) * (T + 4)                  # the smallest such c
    for T in (0, -1, 257, 2 ** 20):
        assert _atlas(10, T) == (-1, (-7, -7, -7))
        with pytest.raises(ValueError):
            TR.atlas_size(10, T)
    for n_faces in (0, -1):
        assert _atlas(n_faces, 8)[0] == -1
    # T = 1: cells of 6 x 5, 2730 per row at most: 2730 * 3276 cells of two faces fit, one more row does not
    most = 2 * 2730 * 3276
    assert _atlas(most, 1) == (0, (2730, 16380, 16380))
    assert _atlas(most + 1, 1)[0] == -5 and _atlas(2 ** 31 - 1, 1)[0] == -5 and _atlas(2 ** 31, 8)[0] == -5 and _atlas(2 ** 40, 8)[0] == -5
    assert _atlas(2 ** 22, 256)[0] == -5
    from ngp_pl_amd import _meshtex_lib
    lib = _meshtex_lib.lib()
    x = C.c_int()
    assert lib.ngp_meshtex_atlas_size(4, 1, None, C.byref(x), C.byref(x)) == -1
    assert lib.ngp_meshtex_atlas_size(4, 1, C.byref(x), None, C.byref(x)) == -1
    assert lib.ngp_meshtex_atlas_size(4, 1, C.byref(x), C.byref(x), None) == -1


# ---- 3. argument validation


def test_argument_validation_needs_no_gpu():
    from ngp_pl_amd import _lib, _meshtex_lib
    lib = _meshtex_lib.lib()
    V, NF, T = 1000, 1800, 4                            # 900 cells of 9 x 8
    _, AW, AH = TR.atlas_size(NF, T)
    W, H, NC = 80, 60, 3
    assert lib.ngp_meshtex_render_workspace_bytes(W, H, NC) == 8 * W * H * NC
    assert lib.ngp_meshtex_render_workspace_bytes(16384, 16384, 2 ** 31 - 1) == 8 * 2 ** 28 * (2 ** 31 - 1)         # 64-bit sizes
    for w, h, n in ((0, H, NC), (W, 0, NC), (-1, H, NC), (16385, H, NC), (W, 16385, NC), (W, H, 0), (W, H, -1), (W, H, 2 ** 31)):
        assert lib.ngp_meshtex_render_workspace_bytes(w, h, n) == 0
    fake = C.c_void_p(4096)          # never dereferenced: every call below is rejected before a launch
    box_ok = (C.c_float * 6)(-1, -1, -1, 1, 1, 1)
    bg_ok = (C.c_float * 3)(1, 1, 1)
    nan, inf = float("nan"), float("inf")
    big = 2 ** 31

    def points(vertices=fake, faces=fake, normals=fake, n_v=V, n_f=NF, t=T, box=box_ok, begin=0, count=AW * AH, p=fake, d=fake, ok=fake):
        return ("ngp_meshtex_texel_points", vertices, faces, normals, n_v, n_f, t, box, begin, count, p, d, ok, None)

    def uvs(n_f=NF, t=T, out=fake):
        return ("ngp_meshtex_face_uvs", n_f, t, out, None)

    def render(vertices=fake, faces=fake, n_v=V, n_f=NF, t=T, texture=fake, K=fake, poses=fake, n_c=NC, w=W, h=H, near=0.01, bg=bg_ok, ws=fake,
               wb=8 * W * H, image=fake, ids=fake, depth=fake):
        return ("ngp_meshtex_render", vertices, faces, n_v, n_f, t, texture, K, poses, n_c, w, h, near, bg, ws, wb, image, ids, depth, None)

    def box(k, x):
        b = [-1, -1, -1, 1, 1, 1]
        b[k] = x
        return (C.c_float * 6)(*b)

    def bg(k, x):
        b = [1, 1, 1]
        b[k] = x
        return (C.c_float * 3)(*b)

    bad = [
        points(vertices=None), points(faces=None), points(normals=None), points(box=None), points(p=None), points(d=None), points(ok=None),
        points(n_v=-1), points(n_f=0), points(n_f=-1), points(t=0), points(t=257), points(t=-3),
        points(begin=-1), points(count=-1), points(begin=1), points(count=AW * AH + 1), points(begin=AW * AH + 1, count=0),
        points(begin=AW * AH, count=1), points(begin=2 ** 62, count=2 ** 62),
        points(box=box(0, nan)), points(box=box(4, nan)), points(box=box(2, -inf)), points(box=box(5, inf)), points(box=box(1, 2.0)),
        uvs(out=None), uvs(n_f=0), uvs(n_f=-5), uvs(t=0), uvs(t=257),
        render(vertices=None), render(faces=None), render(texture=None), render(K=None), render(poses=None), render(bg=None), render(ws=None),
        render(image=None), render(n_v=-1), render(n_f=0), render(n_f=-1), render(t=0), render(t=257), render(n_c=0), render(n_c=-1),
        render(w=0), render(h=0), render(w=-1), render(w=16385), render(h=16385), render(wb=8 * W * H - 1), render(wb=0),
        render(ws=C.c_void_p(4100)),
        render(near=nan), render(near=inf), render(near=-inf), render(bg=bg(0, nan)), render(bg=bg(1, inf)), render(bg=bg(2, -inf)),
    ]
    for args in bad:
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshtex_lib.call(*args)
    too_many = 2 * 2730 * 3276 + 1                      # at T = 1; far fewer at T = 4
    for args in [points(n_v=big), points(n_f=big), points(n_f=too_many, count=1), uvs(n_f=big), uvs(n_f=too_many), uvs(n_f=2 ** 22, t=256),
                 render(n_v=big), render(n_f=big), render(n_f=too_many), render(n_c=big)]:
        with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
            _meshtex_lib.call(*args)
    # nothing to do: no launch
    assert _meshtex_lib.call(*points(count=0)) == 0 and _meshtex_lib.call(*points(begin=AW * AH, count=0)) == 0


# ---- 4. the restatement by hand: T = 1, two faces, one cell of 6 x 5

HAND_V = F([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 1], [4, 2, 1], [2, 4, 1]])
HAND_F = np.int32([[0, 1, 2], [3, 4, 5]])
HAND_OWNER = ["000001", "000011", "000111", "001111", "011111"]
#             slot 0: u = i - 1; slot 1: u = (5 - i) - 1
HAND_U = [[-1, 0, 1, 2, 3, -1], [-1, 0, 1, 2, 0, -1], [-1, 0, 1, 1, 0, -1], [-1, 0, 2, 1, 0, -1], [-1, 3, 2, 1, 0, -1]]
#             slot 0: v = j - 1; slot 1: v = (4 - j) - 1
HAND_VV = [[-1, -1, -1, -1, -1, 3], [0, 0, 0, 0, 2, 2], [1, 1, 1, 1, 1, 1], [2, 2, 0, 0, 0, 0], [3, -1, -1, -1, -1, -1]]


def test_two_faces_by_hand():
    assert TR.atlas_size(2, 1) == (1, 6, 5)
    face, ip, jp = TR.owners(2, 1)
    assert face.reshape(5, 6).tolist() == [[int(ch) for ch in row] for row in HAND_OWNER]
    assert (face == 0).sum() == 15 == (face == 1).sum()
    assert (ip - 1).reshape(5, 6).tolist() == HAND_U and (jp - 1).reshape(5, 6).tolist() == HAND_VV
    normals = np.tile(F([0, 0, 2]), (6, 1))
    p, d, valid = TR.texel_points(HAND_V, HAND_F, normals, 1, (-10, -10, -10, 10, 10, 10))
    assert p.dtype == F and d.dtype == F and valid.dtype == np.uint8 and valid.all()
    # face 0 is the unit triangle at z = 0: the point is (u, v, 0); face 1 has legs of 2 from (2, 2, 1): (2 + 2 u, 2 + 2 v, 1)
    want = [[[u, v, 0] if o == "0" else [2 + 2 * u, 2 + 2 * v, 1] for o, u, v in zip(orow, urow, vrow)] for orow, urow, vrow in zip(HAND_OWNER, HAND_U, HAND_VV)]
    assert p.reshape(5, 6, 3).tolist() == want
    assert (d == F([0, 0, -1])).all() and np.signbit(d).all()                             # -(0 / 2) is -0
    # the corners: a at slot (1, 1), b at (2, 1), c at (1, 2); slot 1 mirrored through (5 - i, 4 - j)
    assert TR.corner_texels(2, 1).tolist() == [[[1, 1], [2, 1], [1, 2]], [[4, 3], [3, 3], [4, 2]]]
    assert p.reshape(5, 6, 3)[1, 1].tolist() == [0, 0, 0] and p.reshape(5, 6, 3)[1, 2].tolist() == [1, 0, 0] and p.reshape(5, 6, 3)[2, 1].tolist() == [0, 1, 0]
    assert p.reshape(5, 6, 3)[3, 4].tolist() == [2, 2, 1] and p.reshape(5, 6, 3)[3, 3].tolist() == [4, 2, 1] and p.reshape(5, 6, 3)[2, 4].tolist() == [2, 4, 1]
    uv = TR.face_uvs(2, 1)
    assert uv.dtype == F and uv.shape == (2, 3, 2)
    want_uv = [[[1.5 / 6, 1 - 1.5 / 5], [2.5 / 6, 1 - 1.5 / 5], [1.5 / 6, 1 - 2.5 / 5]], [[4.5 / 6, 1 - 3.5 / 5], [3.5 / 6, 1 - 3.5 / 5], [4.5 / 6, 1 - 2.5 / 5]]]
    assert np.array_equal(uv, np.asarray(want_uv, np.float64).astype(F))
    # a chunk that begins mid-row is the same texels
    p2, d2, v2 = TR.texel_points(HAND_V, HAND_F, normals, 1, (-10, -10, -10, 10, 10, 10), begin=7, count=11)
    assert np.array_equal(p2, p[7:18]) and np.array_equal(d2, d[7:18]) and np.array_equal(v2, valid[7:18])
    # the clamp, an odd last face, a bad index, a NaN vertex, a zero and a NaN normal
    p3, _, v3 = TR.texel_points(HAND_V, HAND_F, normals, 1, (0, 0, 0, 3, 3, 3))
    assert v3.all() and p3.min() == 0 and p3.max() == 3 and p3.reshape(5, 6, 3)[0, 0].tolist() == [0, 0, 0] and p3.reshape(5, 6, 3)[0, 5].tolist() == [0, 3, 1]
    p4, d4, v4 = TR.texel_points(HAND_V, HAND_F[:1], normals, 1, (-10, -9, -8, 10, 10, 10))
    assert v4.reshape(5, 6).tolist() == [[1 - int(ch) for ch in row] for row in HAND_OWNER]
    assert (p4[v4 == 0] == F([-10, -9, -8])).all() and (d4[v4 == 0] == F([0, 0, 1])).all()
    for bad in (-1, 6):
        _, _, v5 = TR.texel_points(HAND_V, np.int32([[0, 1, bad], [3, 4, 5]]), normals, 1, (-10, -10, -10, 10, 10, 10))
        assert v5.reshape(5, 6).tolist() == [[int(ch) for ch in row] for row in HAND_OWNER]
    vn = HAND_V.copy()
    vn[4, 1] = np.nan
    _, _, v6 = TR.texel_points(vn, HAND_F, normals, 1, (-10, -10, -10, 10, 10, 10))
    assert v6.reshape(5, 6).tolist() == [[1 - int(ch) for ch in row] for row in HAND_OWNER]
    nz = normals.copy()
    nz[:3] = 0
    nz[3:, 0] = np.nan
    _, d7, v7 = TR.texel_points(HAND_V, HAND_F, nz, 1, (-10, -10, -10, 10, 10, 10))
    assert v7.all() and (d7 == F([0, 0, 1])).all() and not np.signbit(d7).any()


# ---- 5. the tiling property


@pytest.mark.parametrize("T", range(1, 10))
def test_bilinear_footprint_stays_in_the_face(T):
    n_faces = 8
    c, W, H = TR.atlas_size(n_faces, T)
    owner = TR.owners(n_faces, T)[0].reshape(H, W)
    n = 12 * T + 7
    b, g = np.meshgrid(np.arange(n + 1) / n, np.arange(n + 1) / n)
    b, g = b.ravel().astype(F), g.ravel().astype(F)
    t = np.linspace(0, 1, 4 * n + 1).astype(F)
    t = t[t >= 0.5]
    # the hypotenuse: 1 - t is exact for t in [0.5, 1]; the corners are its ends and the origin
    b = np.concatenate([b, t, F(1) - t, F([0, 1, 0])])
    g = np.concatenate([g, F(1) - t, t, F([0, 0, 1])])
    keep = b.astype(np.float64) + g.astype(np.float64) <= 1
    b, g = b[keep], g[keep]
    assert len(b) > 70 * T * T and ((b + g) == 1).sum() > 4 * T
    for f in range(n_faces):
        cell = f >> 1
        ox, oy = (cell % c) * (T + 5), (cell // c) * (T + 4)
        _, (i0, i1, j0, j1, fx, fy) = TR.sample(None, T, n_faces, np.full(len(b), f), b, g)
        assert (fx >= 0).all() and (fx < 1).all() and (fy >= 0).all() and (fy < 1).all()
        for i, j, w in ((i0, j0, (1 - fx) * (1 - fy)), (i1, j0, fx * (1 - fy)), (i0, j1, (1 - fx) * fy), (i1, j1, fx * fy)):
            used = w != 0
            assert used.any()
            assert (i[used] >= ox).all() and (i[used] < ox + T + 5).all() and (j[used] >= oy).all() and (j[used] < oy + T + 4).all()
            assert (owner[j[used], i[used]] == f).all()
        # the un-weighted neighbour is still a texel of the atlas: no clamp is needed to stay inside
        assert (i0 + 1 <= W - 1).all() and (j0 + 1 <= H - 1).all() and (i0 >= 0).all() and (j0 >= 0).all()


# ---- 6. a linear colour field, reference only


def test_linear_colour_is_reproduced_within_half_a_step():
    """A colour that is affine in space is affine over every face, the texel points are affine in the slot coordinates and the
    border texels are extrapolated, not clamped (the mesh lies well inside the box): the bilinear lookup of the exact texel colours
    is exact, and what is left is the quantisation, at most half a step of 1 / 255 on each of the four texels and so on their convex
    combination, plus f32 rounding (1e-5 covers the lookup's few operations on values of at most 255 and the points' 1e-7)."""
    v, f, nrm = TR.sphere_mesh(12, radius=0.7, jitter=0.2, seed=0)
    assert 300 < len(f) < 2000 and np.linalg.norm(v, axis=1).max() < 0.8
    T = 4
    box = (-1, -1, -1, 1, 1, 1)
    p, _, valid = TR.texel_points(v, f, nrm, T, box)
    c = TR.linear_colour(p[valid == 1])
    assert c.min() >= 0.05 and c.max() <= 0.95
    texture = TR.bake(v, f, nrm, T, box, TR.linear_colour)
    K, poses, wh = TR.sphere_cameras(3, 48)
    image, ids, depth, beta, gamma = TR.render(v, f, T, texture, K, poses, wh, 0.01, return_weights=True)
    covered = ids >= 0
    assert covered.sum() > 0.3 * covered.size and not covered.all() and (image[~covered] == 1).all() and np.isinf(depth[~covered]).all()
    assert len(np.unique(ids[covered])) > 0.3 * len(f) and (ids[covered] & 1).any() and not (ids[covered] & 1).all()
    tri = v.astype(np.float64)[f[ids[covered]]]
    bb, gg = beta[covered].astype(np.float64)[:, None], gamma[covered].astype(np.float64)[:, None]
    hit = tri[:, 0] + bb * (tri[:, 1] - tri[:, 0]) + gg * (tri[:, 2] - tri[:, 0])
    want = 0.5 + hit @ TR.GRADIENT.T
    err = np.abs(image[covered].astype(np.float64) - want).max()
    print("largest colour error %.6f = %.3f steps of 1/255" % (err, err * 255))
    assert err <= 0.5 / 255 + 1e-5
    # the hit point is where the pixel's ray meets the mesh: at the depth the key holds, along the ray through the pixel centre
    ci, jj, ii = np.nonzero(covered)
    Kd = K.astype(np.float64)
    ray = np.stack([(ii + 0.5 - Kd[0, 2]) / Kd[0, 0], (jj + 0.5 - Kd[1, 2]) / Kd[1, 1], np.ones(len(ii))], 1) * depth[covered].astype(np.float64)[:, None]
    world = np.einsum("nij,nj->ni", poses.astype(np.float64)[ci][:, :, :3], ray) + poses.astype(np.float64)[ci][:, :, 3]
    assert np.abs(world - hit).max() < 1e-4


# ---- 7. OBJ + MTL + PNG


def read_png(path):
    blob = open(path, "rb").read()
    assert blob[:8] == b"\x89PNG\r\n\x1a\n"
    chunks, at = [], 8
    while at < len(blob):
        n, tag = struct.unpack(">I4s", blob[at:at + 8])
        data = blob[at + 8:at + 8 + n]
        assert struct.unpack(">I", blob[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF
        chunks.append((tag, data))
        at += 12 + n
    assert at == len(blob) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, kind, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, kind, comp, filt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(b"".join(d for t, d in chunks if t == b"IDAT")), np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3)


def read_obj(path):
    out = dict(v=[], vn=[], vt=[], f=[], mtllib=[], usemtl=[])
    for line in open(path):
        parts = line.split()
        if not parts or parts[0].startswith("#"):
            continue
        if parts[0] in ("v", "vn", "vt"):
            out[parts[0]].append([float(x) for x in parts[1:]])
        elif parts[0] == "f":
            out["f"].append([[int(x) for x in p.split("/")] for p in parts[1:]])
        else:
            out[parts[0]].append(parts[1])
    return out


def test_save_obj_round_trip(tmp_path):
    from ngp_pl_amd import mesh
    g = np.random.RandomState(5)
    v, f, nrm = TR.sphere_mesh(8, seed=1)
    T = 3
    c, W, H = TR.atlas_size(len(f), T)
    image = g.randint(0, 256, (H, W, 3)).astype(np.uint8)
    tex = mesh.Texture(T, W, H, c, TR.face_uvs(len(f), T), image)
    for normals in (nrm, None):
        m = mesh.Mesh(v, f, normals, None, tex)
        path = str(tmp_path / ("ball%d.obj" % (normals is None)))
        mesh.save_obj(path, m)
        stem = path[:-4]
        assert np.array_equal(read_png(stem + ".png"), image)
        o = read_obj(path)
        assert np.array_equal(np.asarray(o["v"], np.float64).astype(F).view(np.int32), v.view(np.int32))
        assert len(o["vt"]) == 3 * len(f) and np.array_equal(np.asarray(o["vt"], np.float64).astype(F), tex.uvs.reshape(-1, 2))
        faces = np.asarray(o["f"])
        assert faces.shape == (len(f), 3, 3 if normals is not None else 2)
        assert np.array_equal(faces[:, :, 0] - 1, f) and np.array_equal(faces[:, :, 1] - 1, np.arange(3 * len(f)).reshape(-1, 3))
        if normals is not None:
            assert np.array_equal(faces[:, :, 2], faces[:, :, 0]) and np.array_equal(np.asarray(o["vn"], np.float64).astype(F).view(np.int32), nrm.view(np.int32))
        else:
            assert not o["vn"]
        name = os.path.basename(stem)
        assert o["mtllib"] == [name + ".mtl"] and o["usemtl"] == [name]
        mtl = open(stem + ".mtl").read().split()
        assert mtl[mtl.index("newmtl") + 1] == name and mtl[mtl.index("map_Kd") + 1] == name + ".png"
    # a PLY does not see the texture
    a, b = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    colours = g.uniform(0, 1, v.shape).astype(F)
    mesh.save_ply(a, mesh.Mesh(v, f, nrm, colours, tex))
    mesh.save_ply(b, mesh.Mesh(v, f, nrm, colours))
    assert open(a, "rb").read() == open(b, "rb").read()
    for bad in (mesh.Mesh(v, f, nrm), mesh.Mesh(v, f, nrm, None, mesh.Texture(T, W, H, c, tex.uvs)), mesh.Mesh(v, f[:-1], nrm, None, tex)):
        with pytest.raises(ValueError):
            mesh.save_obj(str(tmp_path / "bad.obj"), bad)


# ---- 8. the Python API's checks and the CLI


def test_python_api_argument_checks():
    import torch
    from ngp_pl_amd import mesh
    assert [fl.name for fl in mesh.dataclasses.fields(mesh.Mesh)] == ["vertices", "faces", "normals", "colors", "texture"]
    assert mesh.Mesh(1, 2, 3, 4).texture is None and mesh.Mesh(1, 2).colors is None
    assert [fl.name for fl in mesh.dataclasses.fields(mesh.Texture)] == ["texels", "width", "height", "cells_per_row", "uvs", "image"]
    v = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    m = mesh.Mesh(v, f, torch.zeros(4, 3))
    tex = mesh.Texture(1, 6, 5, 1, torch.zeros(2, 3, 2), torch.zeros(5, 6, 3, dtype=torch.uint8))
    K, poses = np.eye(3, dtype=F), np.zeros((2, 3, 4), F)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.texture_atlas(m)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.texel_points(m, tex, ((0, 0, 0), (1, 1, 1)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.bake_texture(None, m, 1, color_fn=lambda p, d: p, box=((0, 0, 0), (1, 1, 1)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.render_textured(mesh.Mesh(v, f, None, None, tex), K, poses, (8, 8))
    for bad in (f.long(), f.float(), torch.zeros(2, 4, dtype=torch.int32), f.numpy()):
        with pytest.raises(ValueError):
            mesh.texture_atlas(mesh.Mesh(v, bad))
        with pytest.raises(ValueError):
            mesh.render_textured(mesh.Mesh(v, bad, None, None, tex), K, poses, (8, 8))
    with pytest.raises(ValueError):
        mesh.texture_atlas(mesh.Mesh(v.double(), f))
    with pytest.raises(ValueError, match="no faces"):
        mesh.texture_atlas(mesh.Mesh(v, f[:0]))
    with pytest.raises(ValueError, match="no faces"):
        mesh.bake_texture(None, mesh.Mesh(v, f[:0]), 1, color_fn=lambda p, d: p, box=((0, 0, 0), (1, 1, 1)))
    for texels in (0, -1, 257, 2.0, "8", None, True):
        with pytest.raises(ValueError, match="texels"):
            mesh.texture_atlas(m, texels)
        with pytest.raises(ValueError, match="texels"):
            mesh.bake_texture(None, m, texels, color_fn=lambda p, d: p, box=((0, 0, 0), (1, 1, 1)))
        with pytest.raises(ValueError):
            mesh.extract_mesh(None, 8, texture=texels) if texels is not None else mesh.extract_mesh(None, 8, texture=dict(texels=None))
    for texture in (dict(texels=8, border=2), dict(T=8)):
        with pytest.raises(ValueError):
            mesh.extract_mesh(None, 8, texture=texture)
    for chunk in (0, -1, 2.5, None):
        with pytest.raises(ValueError, match="chunk"):
            mesh.bake_texture(None, m, 1, chunk=chunk, color_fn=lambda p, d: p, box=((0, 0, 0), (1, 1, 1)))
    with pytest.raises(ValueError):
        mesh.bake_texture(None, m, 1)                                            # neither a model nor an evaluator
    with pytest.raises(ValueError):
        mesh.render_textured(mesh.Mesh(v, f), K, poses, (0, 8))
    with pytest.raises(ValueError):
        mesh.render_textured(mesh.Mesh(v, f), K, poses[0], (8, 8))


def test_cli_lists_the_option_and_refuses_a_textured_ply(capsys):
    from ngp_pl_amd import mesh
    with pytest.raises(SystemExit) as e:
        mesh.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--texture-texels T" in out and ".obj" in out
    for bad in (["--out", "y.ply", "--texture-texels", "8"], ["--out", "y", "--texture-texels", "8"], ["--out", "y.obj"],
                ["--out", "y.obj", "--texture-texels", "0"], ["--out", "y.obj", "--texture-texels", "257"],
                ["--out", "y.obj", "--texture-texels", "2.5"]):
        with pytest.raises(SystemExit) as e:
            mesh.main(["--ckpt", "x"] + bad)
        assert e.value.code == 2
    assert "--texture-texels" in capsys.readouterr().err
