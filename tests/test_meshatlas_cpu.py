"""CPU: the C ABI of libngp_meshatlas.so (header, exports, ctypes, code object, build entry, the host-only layout against hand
answers and the restatement, host-side refusals of every entry point), the Python API's and the CLI's argument checks, the OBJ
writer with an AdaptiveTexture, and the numpy restatement the GPU tests compare against (tests/mesh_atlas_reference.py): class
thresholds hit exactly, the tiling property of the bilinear footprint for every ladder value, and an affine colour on a mesh of
mixed classes within half a quantisation step."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_atlas_reference as AR
from tests import mesh_texture_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN = os.path.join(ROOT, "ngp_pl_amd", "csrc", "meshatlas")            # the header lies beside the sources
HEADER = os.path.join(OWN, "ngp_meshatlas.h")
OTHERS = ("ngp_hip.h", "ngp_mesh.h", "ngp_meshfilter.h", "ngp_meshcull.h", "ngp_meshsimplify.h", "ngp_meshtsdf.h", "ngp_meshsmooth.h",
          "ngp_meshtex.h", "ngp_metrics.h", "ngp_meshdist.h", "ngp_meshquadric.h", "ngp_meshdecimate.h")
ENTRY_POINTS = ("abi_version", "build_arch", "classify_workspace_bytes", "classify", "layout", "place", "texel_points", "face_uvs",
                "render_workspace_bytes", "render")
F = np.float32


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


# ---- 1. the C ABI


def test_header_compiles_as_c99_alone_and_beside_the_other_twelve_in_several_orders():
    assert len(set(OTHERS)) == 12 and set(OTHERS) <= set(os.listdir(os.path.join(ROOT, "include"))) and os.path.exists(HEADER)
    inc = lambda names: "".join('#include "%s"\n' % n for n in names)
    for src in ('#include "ngp_meshatlas.h"\nint main(void) { return 0; }\n',
                inc(OTHERS + ("ngp_meshatlas.h",)) + "int main(void) { return NGP_EINVAL + NGP_ERANGE + NGP_MESHATLAS_CLASSES; }\n",
                inc(("ngp_meshatlas.h",) + OTHERS[::-1]) + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n",
                inc(OTHERS[5:] + ("ngp_meshatlas.h",) + OTHERS[:5]) + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n"):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-I", OWN, "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}
    assert "#ifndef NGP_EINVAL" in text and "#ifndef NGP_ERANGE" in text and "THE RULE" in text
    # the ladder of THE RULE is the restatement's and the binding's
    from ngp_pl_amd import _meshatlas_lib
    assert ", ".join(str(t) for t in AR.LADDER) in text and AR.LADDER == _meshatlas_lib.LADDER and len(AR.LADDER) == 16


def test_library_exports_exactly_its_header():
    from ngp_pl_amd import _abi, _meshatlas_lib
    protos = _abi.parse(HEADER)
    assert set(protos) == {"ngp_meshatlas_" + n for n in ENTRY_POINTS}
    assert _exports(_meshatlas_lib.LIB_PATH) == set(protos)
    assert set(_meshatlas_lib.exported_symbols()) == set(protos)
    lib = _meshatlas_lib.lib()
    assert lib.ngp_meshatlas_abi_version() == 1 == _meshatlas_lib.ABI_VERSION and lib.ngp_meshatlas_build_arch() == b"gfx950"


def test_the_thirteen_libraries_share_no_symbol():
    from ngp_pl_amd import (_abi, _lib, _mesh_lib, _meshatlas_lib, _meshcull_lib, _meshdecimate_lib, _meshdist_lib, _meshfilter_lib,
                            _meshquadric_lib, _meshsimplify_lib, _meshsmooth_lib, _meshtex_lib, _meshtsdf_lib, _metrics_lib)
    mods = (_lib, _mesh_lib, _meshfilter_lib, _meshcull_lib, _meshsimplify_lib, _meshtsdf_lib, _meshsmooth_lib, _meshtex_lib, _metrics_lib,
            _meshdist_lib, _meshquadric_lib, _meshdecimate_lib, _meshatlas_lib)
    assert len({m.LIB_PATH for m in mods}) == 13
    exports = [_exports(m.LIB_PATH) for m in mods]
    assert all(exports)
    for i, a in enumerate(exports):
        for b in exports[i + 1:]:
            assert not a & b
    own, others = exports[-1], set().union(*exports[:-1])
    assert not [s for s in others if s.startswith("ngp_meshatlas")]
    assert not [s for s in own if not s.startswith("ngp_meshatlas_")]
    declared = set(_abi.parse(HEADER))
    for h in OTHERS:
        assert not declared & set(_abi.parse(os.path.join(ROOT, "include", h))), h


def test_ctypes_agrees_with_the_header():
    from ngp_pl_amd import _abi, _meshatlas_lib
    protos = _abi.parse(HEADER)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _meshatlas_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    lib = _meshatlas_lib.lib()
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        want = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret]
        assert f.restype is want, name


def test_code_object_is_gfx950_only():
    from ngp_pl_amd import _meshatlas_lib
    blob = open(_meshatlas_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob
    for kernel in (b"atlas_count", b"atlas_scan", b"atlas_scatter", b"atlas_place", b"atlas_points", b"atlas_uvs", b"atlas_raster", b"atlas_shade"):
        assert kernel in blob


def test_build_links_the_thirteenth_library_with_contraction_off():
    from ngp_pl_amd import _meshatlas_lib, build
    assert build.MESHATLAS_LIB == _meshatlas_lib.LIB_PATH and build.MESHATLAS_CFLAGS == ["-ffp-contract=off"]
    assert build.ARCH == "gfx950" and build.MESHATLAS_SOURCES == [os.path.join("meshatlas", "meshatlas.hip")]
    for rel in build.MESHATLAS_SOURCES + build.MESHATLAS_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, rel)), rel
    # no ABI header or source of the uniform atlas's library is compiled into this one: only the shared camera and raster device code,
    # the integer scans and the host helpers every mesh library shares
    source = open(os.path.join(build.CSRC, build.MESHATLAS_SOURCES[0])).read()
    assert set(re.findall(r'#include\s*"([^"]+)"', source)) == {"ngp_meshatlas.h", "../mesh_camera.h", "../mesh_raster.h", "../mesh_host.h",
                                                                 "../mesh_scan.h"}


# ---- 2. the layout against hand answers and the restatement


def _layout(counts):
    from ngp_pl_amd import _meshatlas_lib
    arr = (C.c_int64 * 16)(*counts)
    w, h = C.c_int(-7), C.c_int(-7)
    bands = (C.c_int32 * 64)(*([-7] * 64))
    rc = _meshatlas_lib.lib().ngp_meshatlas_layout(arr, C.byref(w), C.byref(h), bands)
    return rc, (w.value, h.value), [tuple(bands[4 * c:4 * c + 4]) for c in range(16)]


def only(c, n):
    counts = [0] * 16
    counts[c] = n
    return counts


def test_layout_hand_answers():
    # one face of class 15: one cell of 261 x 260
    assert _layout(only(15, 1)) == (0, (261, 260), [(0, 0, 0, 0)] * 15 + [(0, 260, 1, 1)])
    # 3 faces of class 8 (T = 24, cells of 29 x 28): two cells, the last slot empty; one per row until W = 58, and 56 >= 2 * 28
    rc, wh, bands = _layout(only(8, 3))
    assert (rc, wh, bands[8]) == (0, (56, 56), (0, 56, 1, 2)) and AR.layout(only(8, 3))[:2] == (56, 56)
    owner = AR.owners(np.arange(3), only(8, 3))[0].reshape(56, 56)
    assert set(np.unique(owner).tolist()) == {-1, 0, 1, 2} and (owner[28:] != 1).all() and (owner[:, 29:] == -1).all()
    assert (owner == 2).sum() == 29 * 28 // 2 == (owner == 0).sum() and (owner[28:, :29] == -1).sum() == 29 * 28 // 2
    # all 16 classes, one face each: sixteen bands of one cell and one row, whatever the width: H = sum of (T + 4) = 956 = W
    rc, wh, bands = _layout([1] * 16)
    assert (rc, wh) == (0, (956, 956)) and sum(AR.LADDER) + 64 == 956
    y = 0
    for c in range(15, -1, -1):
        assert bands[c] == (y, AR.LADDER[c] + 4, 956 // (AR.LADDER[c] + 5), 1)
        y += AR.LADDER[c] + 4
    # class 5 (T = 8, cells of 13 x 12): 100 cells fill 10 rows of 10 exactly (130 x 120; 9 per row need 12 rows = 144 > 129);
    # one cell more needs an eleventh row: 132 high, and 132 wide is still 10 per row
    assert _layout(only(5, 200))[:2] == (0, (130, 120)) and _layout(only(5, 200))[2][5] == (0, 120, 10, 100)
    assert _layout(only(5, 201))[:2] == (0, (132, 132)) and _layout(only(5, 202))[2][5] == (0, 132, 10, 101)
    # class 0 (T = 1, cells of 6 x 5): 2730 per row and 3276 rows fit 16384, one face more does not
    most = 2 * 2730 * 3276
    assert _layout(only(0, most))[:2] == (0, (16380, 16380))
    assert _layout(only(0, most + 1)) == (-5, (-7, -7), [(-7, -7, -7, -7)] * 16)
    with pytest.raises(OverflowError):
        AR.layout(only(0, most + 1))
    assert _layout(only(3, 2 ** 31))[0] == -5 and _layout([2 ** 30] * 16)[0] == -5 and _layout(only(15, 2 ** 24))[0] == -5
    for bad in ([0] * 16, only(4, -1), [5] * 15 + [-1]):
        assert _layout(bad)[0] == -1
        with pytest.raises(ValueError):
            AR.layout(bad)
    from ngp_pl_amd import _meshatlas_lib
    lib, x = _meshatlas_lib.lib(), C.c_int()
    ok = (C.c_int64 * 16)(*only(2, 4))
    assert lib.ngp_meshatlas_layout(None, C.byref(x), C.byref(x), None) == -1 and lib.ngp_meshatlas_layout(ok, None, C.byref(x), None) == -1
    assert lib.ngp_meshatlas_layout(ok, C.byref(x), None, None) == -1 and lib.ngp_meshatlas_layout(ok, C.byref(x), C.byref(x), None) == 0


def test_layout_against_the_restatement():
    g = np.random.RandomState(11)
    cases = [[2 * k + 1 for k in range(16)], [2 * (15 - k) + 1 for k in range(16)], [101] * 16, only(0, 1), only(0, 2), only(7, 65537)]
    for _ in range(150):
        c = (g.randint(0, 2, 16) * g.randint(0, 10 ** g.randint(1, 6), 16)).tolist()
        if sum(c):
            cases.append(c)
    for counts in cases:
        try:
            want = AR.layout(counts)
        except OverflowError:
            assert _layout(counts)[0] == -5
            continue
        rc, (w, h), bands = _layout(counts)
        assert rc == 0 and (w, h, bands) == want, counts
        top = max(c for c in range(16) if counts[c])
        assert h <= w <= 16384 and w >= AR.LADDER[top] + 5 and (w == AR.LADDER[top] + 5 or AR.height_at(counts, w - 1) > w - 1)
        assert h == sum(b[1] for b in bands)
        # every face has a cell of its own band, inside the atlas
        place = AR.place(np.arange(sum(counts)), counts) if sum(counts) < 5000 else None
        if place is not None:
            ox, oy, c, slot, T = AR.decode(place)
            assert (ox + T + 5 <= w).all() and (oy + T + 4 <= h).all() and len({(a, b, s) for a, b, s in zip(ox, oy, slot)}) == len(ox)
            assert np.array_equal(np.bincount(c, minlength=16), counts)


# ---- 3. host refusals, no GPU


def test_argument_validation_needs_no_gpu():
    from ngp_pl_amd import _lib, _meshatlas_lib
    lib = _meshatlas_lib.lib()
    V, NF = 1000, 1800
    counts = [0] * 16
    counts[3], counts[6] = 1000, 800
    AW, AH, _ = AR.layout(counts)
    W, H, NCAM = 80, 60, 3
    assert lib.ngp_meshatlas_render_workspace_bytes(W, H, NCAM) == 8 * W * H * NCAM
    for w, h, n in ((0, H, NCAM), (W, 0, NCAM), (-1, H, NCAM), (16385, H, NCAM), (W, 16385, NCAM), (W, H, 0), (W, H, -1), (W, H, 2 ** 31)):
        assert lib.ngp_meshatlas_render_workspace_bytes(w, h, n) == 0
    ws_bytes = lib.ngp_meshatlas_classify_workspace_bytes(NF)
    assert ws_bytes > 0 and ws_bytes % 256 == 0 and lib.ngp_meshatlas_classify_workspace_bytes(40 * 2048 + 1) >= 41 * 16 * 12 > lib.ngp_meshatlas_classify_workspace_bytes(2048) >= 16 * 12
    for n in (0, -1, 2 ** 31):
        assert lib.ngp_meshatlas_classify_workspace_bytes(n) == 0
    assert lib.ngp_meshatlas_classify_workspace_bytes(2 ** 31 - 1) >= 16 * 12 * 2 ** 20
    fake = C.c_void_p(4096)          # never dereferenced: every call below is rejected before a launch
    box_ok = (C.c_float * 6)(-1, -1, -1, 1, 1, 1)
    bg_ok = (C.c_float * 3)(1, 1, 1)
    cnt_ok = (C.c_int64 * 16)(*counts)
    nan, inf = float("nan"), float("inf")
    big = 2 ** 31

    def cnt(c, n):
        x = list(counts)
        x[c] = n
        return (C.c_int64 * 16)(*x)

    def classify(vertices=fake, faces=fake, n_v=V, n_f=NF, s=0.01, cmin=0, cmax=15, cls=fake, order=fake, out=fake, ws=fake, wb=ws_bytes):
        return ("ngp_meshatlas_classify", vertices, faces, n_v, n_f, s, cmin, cmax, cls, order, out, ws, wb, None)

    def place(order=fake, c=cnt_ok, n_f=NF, out=fake):
        return ("ngp_meshatlas_place", order, c, n_f, out, None)

    def points(vertices=fake, faces=fake, normals=fake, n_v=V, n_f=NF, order=fake, c=cnt_ok, box=box_ok, begin=0, count=AW * AH, p=fake, d=fake, ok=fake):
        return ("ngp_meshatlas_texel_points", vertices, faces, normals, n_v, n_f, order, c, box, begin, count, p, d, ok, None)

    def uvs(fp=fake, n_f=NF, w=AW, h=AH, out=fake):
        return ("ngp_meshatlas_face_uvs", fp, n_f, w, h, out, None)

    def render(vertices=fake, faces=fake, n_v=V, n_f=NF, fp=fake, texture=fake, aw=AW, ah=AH, K=fake, poses=fake, n_c=NCAM, w=W, h=H, near=0.01,
               bg=bg_ok, ws=fake, wb=8 * W * H, image=fake, ids=fake, depth=fake):
        return ("ngp_meshatlas_render", vertices, faces, n_v, n_f, fp, texture, aw, ah, K, poses, n_c, w, h, near, bg, ws, wb, image, ids, depth, None)

    def box(k, x):
        b = [-1, -1, -1, 1, 1, 1]
        b[k] = x
        return (C.c_float * 6)(*b)

    def bg(k, x):
        b = [1, 1, 1]
        b[k] = x
        return (C.c_float * 3)(*b)

    bad = [
        classify(vertices=None), classify(faces=None), classify(cls=None), classify(order=None), classify(out=None), classify(ws=None),
        classify(n_v=-1), classify(n_f=0), classify(n_f=-1), classify(s=0.0), classify(s=-0.0), classify(s=-1.0), classify(s=nan), classify(s=inf),
        classify(s=-inf), classify(cmin=-1), classify(cmax=16), classify(cmin=5, cmax=4), classify(cmin=16, cmax=16), classify(wb=ws_bytes - 1),
        classify(wb=0), classify(ws=C.c_void_p(4100)), classify(out=C.c_void_p(4100)),
        place(order=None), place(c=None), place(out=None), place(n_f=0), place(n_f=-1), place(n_f=NF + 1), place(n_f=NF - 1), place(c=cnt(3, -1)),
        points(vertices=None), points(faces=None), points(normals=None), points(order=None), points(c=None), points(box=None), points(p=None),
        points(d=None), points(ok=None), points(n_v=-1), points(n_f=0), points(n_f=-1), points(n_f=NF + 1), points(c=cnt(0, 1)), points(c=cnt(6, -800)),
        points(begin=-1), points(count=-1), points(begin=1), points(count=AW * AH + 1), points(begin=AW * AH + 1, count=0),
        points(begin=AW * AH, count=1), points(begin=2 ** 62, count=2 ** 62),
        points(box=box(0, nan)), points(box=box(4, nan)), points(box=box(2, -inf)), points(box=box(5, inf)), points(box=box(1, 2.0)),
        uvs(fp=None), uvs(out=None), uvs(n_f=0), uvs(n_f=-5), uvs(w=0), uvs(h=0), uvs(w=16385), uvs(h=16385), uvs(w=-1),
        render(vertices=None), render(faces=None), render(fp=None), render(texture=None), render(K=None), render(poses=None), render(bg=None),
        render(ws=None), render(image=None), render(n_v=-1), render(n_f=0), render(n_f=-1), render(aw=0), render(ah=0), render(aw=16385),
        render(ah=16385), render(n_c=0), render(n_c=-1), render(w=0), render(h=0), render(w=-1), render(w=16385), render(h=16385),
        render(wb=8 * W * H - 1), render(wb=0), render(ws=C.c_void_p(4100)),
        render(near=nan), render(near=inf), render(near=-inf), render(bg=bg(0, nan)), render(bg=bg(1, inf)), render(bg=bg(2, -inf)),
    ]
    for args in bad:
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshatlas_lib.call(*args)
    too_many = 2 * 2730 * 3276 + 1
    for args in [classify(n_v=big), classify(n_f=big), place(c=cnt(0, too_many), n_f=too_many + NF), points(n_v=big),
                 points(c=cnt(0, too_many), n_f=too_many + NF, count=1), uvs(n_f=big), render(n_v=big), render(n_f=big), render(n_c=big)]:
        with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
            _meshatlas_lib.call(*args)
    # nothing to do: no launch
    assert _meshatlas_lib.call(*points(count=0)) == 0 and _meshatlas_lib.call(*points(begin=AW * AH, count=0)) == 0


# ---- 4. the restatement: thresholds, order, place


def test_class_thresholds_are_hit_exactly():
    """s = 2^-6 and an edge of T_c * 2^-6: every number is a small dyadic rational, m = t * t holds bit for bit and gives class c; the
    next float up in the edge gives c + 1 (class 15 stays 15)."""
    s = F(2.0 ** -6)
    for c, T in enumerate(AR.LADDER):
        L = F(T) * s
        up = np.nextafter(L, F(np.inf))
        for k, (e, want) in enumerate(((L, c), (up, min(c + 1, 15)))):
            # the longest edge as ab, bc and ca in turn, the others shorter
            p, q, r = [0, 0, 0], [e, 0, 0], [e / 2, e / 8, 0]           # pq = e, the other two edges e * sqrt(17) / 8
            v = F([p, q, r, r, p, q, q, r, p])
            f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
            assert AR.face_classes(v, f, s).tolist() == [want] * len(f), (c, k)
        assert AR.face_classes(F([[0, 0, 0], [L, 0, 0], [0, L, 0]]), [[0, 1, 2]], s).tolist() == [min([k for k in range(16) if AR.LADDER[k] >= T * 2 ** 0.5] + [15])]   # the hypotenuse L sqrt(2)
    v = F([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [np.nan, 0, 0], [np.inf, 0, 0], [3e38, 0, 0], [-3e38, 0, 0]])
    f = np.int32([[0, 1, 2], [0, 0, 0], [0, 1, -1], [0, 1, 7], [0, 1, 3], [3, 1, 2], [0, 1, 4], [5, 6, 0], [1, 0, 2]])
    # 0.1414 / 2^-6 = 9.05 -> T = 12 (class 6); zero length: the smallest class; bad indices, a NaN in a or b, inf and an overflowing e: cmin; a NaN in c alone leaves e_ab
    assert AR.face_classes(v, f, s).tolist() == [6, 0, 0, 0, 5, 0, 0, 0, 6]
    assert AR.face_classes(v, f, s, 2, 5).tolist() == [5, 2, 2, 2, 5, 2, 2, 2, 5] and AR.face_classes(v, f, s, 7, 7).tolist() == [7] * 9
    # a NaN only in vertex c: e_ab alone decides, as the rule's two comparisons say
    assert AR.face_classes(v, np.int32([[0, 1, 3]]), s, 1, 15).tolist() == [5]                 # 0.1 / 2^-6 = 6.4 -> T = 8
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            AR.face_classes(v, f, bad)
    with pytest.raises(ValueError):
        AR.face_classes(v, f, s, 5, 4)


def test_order_and_place_by_hand():
    cls = np.uint8([3, 0, 3, 15, 0, 3, 2])
    order, counts = AR.sort_faces(cls)
    assert order.tolist() == [3, 0, 2, 5, 6, 1, 4] and counts.tolist() == [2, 0, 1, 3] + [0] * 11 + [1]
    assert AR.bases(counts).tolist() == [5, 5, 4, 1] + [1] * 11 + [0]
    W, H, bands = AR.layout(counts)
    # bands of 260, 8 (T = 4: two cells in a row), 7 (T = 3) and 5 (T = 1) rows: H = 280, and W = 280 >= 261
    assert (W, H) == (280, 280) and [bands[c][0] for c in (15, 3, 2, 0)] == [0, 260, 268, 275]
    place = AR.place(order, counts)
    ox, oy, c, slot, T = AR.decode(place)
    assert c.tolist() == cls.tolist() and T.tolist() == [4, 1, 4, 256, 1, 4, 3]
    assert list(zip(ox.tolist(), oy.tolist(), slot.tolist())) == [(0, 260, 0), (0, 275, 0), (0, 260, 1), (0, 0, 0), (0, 275, 1), (9, 260, 0), (0, 268, 0)]
    owner = AR.owners(order, counts)[0].reshape(H, W)
    for f in range(7):
        i, j = AR.corner_texels(place)[f, 0]
        assert owner[j, i] == f
    assert (owner[:260, 261:] == -1).all() and (owner[260:268, 18:] == -1).all() and set(np.unique(owner[260:268, 9:18]).tolist()) == {-1, 5}
    uv = AR.face_uvs(place, W, H)
    assert uv.dtype == F and uv[3].tolist() == [[F(1.5 / 280), F(1 - 1.5 / 280)], [F(257.5 / 280), F(1 - 1.5 / 280)], [F(1.5 / 280), F(1 - 257.5 / 280)]]


# ---- 5. the tiling property for every ladder value


@pytest.mark.parametrize("c", range(16))
def test_bilinear_footprint_stays_in_the_face(c):
    T = AR.LADDER[c]
    counts = [0] * 16
    counts[c] = 5
    counts[(c + 5) % 16] = 3                             # a band of another class above or below
    cls = np.uint8([c, (c + 5) % 16, c, c, (c + 5) % 16, c, (c + 5) % 16, c])
    order, counts = AR.sort_faces(cls)
    W, H, _ = AR.layout(counts)
    place = AR.place(order, counts)
    owner = AR.owners(order, counts)[0].reshape(H, W)
    n = min(12 * T + 7, 400)
    b, g = np.meshgrid(np.arange(n + 1) / n, np.arange(n + 1) / n)
    b, g = b.ravel().astype(F), g.ravel().astype(F)
    t = np.linspace(0, 1, 4 * n + 1).astype(F)
    t = t[t >= 0.5]
    # the hypotenuse: 1 - t is exact for t in [0.5, 1]; the corners are its ends and the origin
    b = np.concatenate([b, t, F(1) - t, F([0, 1, 0])])
    g = np.concatenate([g, F(1) - t, t, F([0, 0, 1])])
    keep = b.astype(np.float64) + g.astype(np.float64) <= 1
    b, g = b[keep], g[keep]
    assert ((b + g) == 1).sum() > 4 * min(T, 30)
    ox, oy, _, _, Tf = AR.decode(place)
    for f in np.nonzero(cls == c)[0]:
        _, (i0, i1, j0, j1, fx, fy) = AR.sample(None, place, W, H, np.full(len(b), f), b, g)
        assert (fx >= 0).all() and (fx < 1).all() and (fy >= 0).all() and (fy < 1).all()
        for i, j, w in ((i0, j0, (1 - fx) * (1 - fy)), (i1, j0, fx * (1 - fy)), (i0, j1, (1 - fx) * fy), (i1, j1, fx * fy)):
            used = w != 0
            assert used.any()
            assert (i[used] >= ox[f]).all() and (i[used] < ox[f] + T + 5).all() and (j[used] >= oy[f]).all() and (j[used] < oy[f] + T + 4).all()
            assert (owner[j[used], i[used]] == f).all()
        # the un-weighted neighbour is still a texel of the atlas: the clamps change nothing for a record of the rule
        assert (i0 + 1 <= W - 1).all() and (j0 + 1 <= H - 1).all() and (i0 >= 0).all() and (j0 >= 0).all()


# ---- 6. an affine colour on a mesh of mixed classes, reference only


def test_linear_colour_is_reproduced_within_half_a_step():
    """The derivation of tests/test_meshtex_cpu.py's test of the same name holds face by face, whatever T a face has: a colour that is
    affine in space is affine over every face, the texel points are affine in the slot coordinates and the border is extrapolated
    (the mesh lies well inside the box), so the bilinear lookup of the exact texel colours is exact; what is left is the
    quantisation, at most half a step of 1 / 255 on each of the four texels and so on their convex combination, plus f32 rounding
    (1e-5)."""
    v, f, nrm = TR.sphere_mesh(12, radius=0.7, jitter=0.2, seed=0)
    atlas = AR.Atlas(v, f, 0.04)
    used = np.nonzero(atlas.counts)[0]
    assert len(used) >= 3 and atlas.counts.max() < 0.8 * len(f), atlas.counts
    box = (-1, -1, -1, 1, 1, 1)
    texture = AR.bake(v, f, nrm, atlas, box, TR.linear_colour)
    K, poses, wh = TR.sphere_cameras(3, 48)
    image, ids, depth, beta, gamma = AR.render(v, f, atlas.face_place, texture, K, poses, wh, 0.01, return_weights=True)
    covered = ids >= 0
    assert covered.sum() > 0.3 * covered.size and not covered.all() and (image[~covered] == 1).all() and np.isinf(depth[~covered]).all()
    assert len(np.unique(atlas.face_class[ids[covered]])) >= 3
    tri = v.astype(np.float64)[f[ids[covered]]]
    bb, gg = beta[covered].astype(np.float64)[:, None], gamma[covered].astype(np.float64)[:, None]
    hit = tri[:, 0] + bb * (tri[:, 1] - tri[:, 0]) + gg * (tri[:, 2] - tri[:, 0])
    err = np.abs(image[covered].astype(np.float64) - (0.5 + hit @ TR.GRADIENT.T)).max()
    print("largest colour error %.6f = %.3f steps of 1/255" % (err, err * 255))
    assert err <= 0.5 / 255 + 1e-5
    # no face is sampled coarser than the texel size, and one class lower would be
    spacing = AR.face_spacing(v, f, atlas.face_texels)
    assert spacing.max() <= 0.04 * (1 + 1e-6)
    lower = np.asarray(AR.LADDER)[np.maximum(atlas.face_class.astype(int) - 1, 0)]
    assert (AR.longest_edges(v, f)[atlas.face_class > 0] / lower[atlas.face_class > 0] > 0.04 * (1 - 1e-6)).all()


# ---- 7. OBJ + MTL + PNG with an AdaptiveTexture


def test_save_obj_round_trip(tmp_path):
    from ngp_pl_amd import mesh
    from tests.test_meshtex_cpu import read_obj, read_png
    g = np.random.RandomState(5)
    v, f, nrm = TR.sphere_mesh(8, seed=1)
    a = AR.Atlas(v, f, 0.05)
    assert (a.counts > 0).sum() >= 2
    image = g.randint(0, 256, (a.H, a.W, 3)).astype(np.uint8)
    tex = mesh.AdaptiveTexture(0.05, 1, 256, a.W, a.H, tuple(a.counts.tolist()), a.order, a.face_place, a.face_texels.astype(np.int32), a.uvs, image)
    for normals in (nrm, None):
        m = mesh.Mesh(v, f, normals, None, tex)
        path = str(tmp_path / ("ball%d.obj" % (normals is None)))
        mesh.save_obj(path, m)
        stem = path[:-4]
        assert np.array_equal(read_png(stem + ".png"), image)
        o = read_obj(path)
        assert np.array_equal(np.asarray(o["v"], np.float64).astype(F).view(np.int32), v.view(np.int32))
        assert len(o["vt"]) == 3 * len(f) and np.array_equal(np.asarray(o["vt"], np.float64).astype(F), a.uvs.reshape(-1, 2))
        faces = np.asarray(o["f"])
        assert faces.shape == (len(f), 3, 3 if normals is not None else 2)
        assert np.array_equal(faces[:, :, 0] - 1, f) and np.array_equal(faces[:, :, 1] - 1, np.arange(3 * len(f)).reshape(-1, 3))
        name = os.path.basename(stem)
        assert o["mtllib"] == [name + ".mtl"] and o["usemtl"] == [name]
    # every vt is the centre of the texel that holds its corner: the face's own texel
    owner = AR.owners(a.order, a.counts)[0].reshape(a.H, a.W)
    uv = a.uvs.astype(np.float64)
    gi, gj = np.floor(uv[..., 0] * a.W).astype(int), np.floor((1 - uv[..., 1]) * a.H).astype(int)
    assert (owner[gj, gi] == np.arange(len(f))[:, None]).all()
    with pytest.raises(ValueError):
        mesh.save_obj(str(tmp_path / "bad.obj"), mesh.Mesh(v, f, nrm, None, mesh.dataclasses.replace(tex, image=None)))


# ---- 8. the Python API's checks and the CLI


def test_python_api_argument_checks():
    import torch
    from ngp_pl_amd import mesh
    assert [fl.name for fl in mesh.dataclasses.fields(mesh.AdaptiveTexture)] == ["texel_size", "min_texels", "max_texels", "width", "height", "counts",
                                                                                "order", "face_place", "face_texels", "uvs", "image"]
    v = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    m = mesh.Mesh(v, f, torch.zeros(4, 3))
    box = ((0, 0, 0), (1, 1, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.texture_atlas(m, texel_size=0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.fit_texel_size(m, 64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.bake_texture(None, m, texel_size=0.1, color_fn=lambda p, d: p, box=box)
    for texels in (4, 1, 9, 0, "8", None, 8.0, True):
        with pytest.raises(ValueError, match="texels"):
            mesh.texture_atlas(m, texels, texel_size=0.1)
        with pytest.raises(ValueError, match="texels"):
            mesh.bake_texture(None, m, texels, color_fn=lambda p, d: p, box=box, texel_size=0.1)
    for size in (0, 0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60, "1", True, (1,)):
        with pytest.raises(ValueError, match="texel_size"):
            mesh.texture_atlas(m, texel_size=size)
        with pytest.raises(ValueError):
            mesh.extract_mesh(None, 8, texture=dict(texel_size=size))
    for lo, hi in ((5, 256), (1, 255), (0, 8), (1, 512), (16, 8), (2.0, 8), (True, 8), (None, 8), (1, None)):
        with pytest.raises(ValueError, match="texels"):
            mesh.texture_atlas(m, texel_size=0.1, min_texels=lo, max_texels=hi)
        with pytest.raises(ValueError, match="texels"):
            mesh.fit_texel_size(m, 64, lo, hi)
        with pytest.raises(ValueError):
            mesh.extract_mesh(None, 8, texture=dict(texel_size=1.0, min_texels=lo, max_texels=hi))
    for side in (0, -1, 16385, 2.5, None, True):
        with pytest.raises(ValueError, match="max_side"):
            mesh.fit_texel_size(m, side)
        with pytest.raises(ValueError):
            mesh.extract_mesh(None, 8, texture=dict(max_side=side))
    for probes in (0, -1, 2.5, None):
        with pytest.raises(ValueError, match="probes"):
            mesh.fit_texel_size(m, 64, probes=probes)
    for texture in (dict(texel_size=1.0, texels=8), dict(texel_size=1.0, max_side=64), dict(max_side=64, texels=4), dict(min_texels=2),
                    dict(texels=8, max_texels=16), dict(texel_size=1.0, border=2)):
        with pytest.raises(ValueError):
            mesh.extract_mesh(None, 8, texture=texture)
    with pytest.raises(ValueError, match="no faces"):
        mesh.texture_atlas(mesh.Mesh(v, f[:0]), texel_size=0.1)
    with pytest.raises(ValueError, match="no faces"):
        mesh.fit_texel_size(mesh.Mesh(v, f[:0]), 64)


def test_cli_lists_the_options_and_refuses_bad_combinations(capsys):
    from ngp_pl_amd import mesh
    with pytest.raises(SystemExit) as e:
        mesh.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--texture-texel-size VOXELS", "--texture-max-side N", "--texture-min-texels T", "--texture-max-texels T", "--texture-texels T"):
        assert flag in out
    for bad in (["--out", "y.obj", "--texture-texels", "8", "--texture-texel-size", "1"], ["--out", "y.obj", "--texture-texels", "8", "--texture-max-side", "512"],
                ["--out", "y.obj", "--texture-texel-size", "1", "--texture-max-side", "512"], ["--out", "y.ply", "--texture-texel-size", "1"],
                ["--out", "y.ply", "--texture-max-side", "512"], ["--out", "y.obj", "--texture-texel-size", "0"], ["--out", "y.obj", "--texture-texel-size", "-2"],
                ["--out", "y.obj", "--texture-texel-size", "nan"], ["--out", "y.obj", "--texture-texel-size", "inf"], ["--out", "y.obj", "--texture-max-side", "0"],
                ["--out", "y.obj", "--texture-max-side", "16385"], ["--out", "y.obj", "--texture-max-side", "2.5"],
                ["--out", "y.obj", "--texture-texel-size", "1", "--texture-min-texels", "5"], ["--out", "y.obj", "--texture-texel-size", "1", "--texture-max-texels", "100"],
                ["--out", "y.obj", "--texture-texel-size", "1", "--texture-min-texels", "16", "--texture-max-texels", "8"],
                ["--out", "y.obj", "--texture-texels", "8", "--texture-min-texels", "2"], ["--out", "y.obj", "--texture-max-texels", "64"],
                ["--out", "y.obj"]):
        with pytest.raises(SystemExit) as e:
            mesh.main(["--ckpt", "x"] + bad)
        assert e.value.code == 2, bad
        assert "--texture-" in capsys.readouterr().err
