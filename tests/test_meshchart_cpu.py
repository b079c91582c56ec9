"""CPU: the C ABI of libngp_meshchart.so (header, exports, ctypes, code object, build entry, host-side refusals of every entry
point), the host-only packer against hand answers and the restatement, the Python API's and the CLI's argument checks, the GLB
writer, and the numpy restatement the GPU tests compare against (tests/mesh_chart_reference.py): the charts of the scenes and the
properties every atlas of the rule has."""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import mesh_atlas_reference as AR
from tests import mesh_chart_reference as CR
from tests import mesh_normal_reference as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN = os.path.join(ROOT, "ngp_pl_amd", "csrc", "meshchart")            # the header lies beside the sources
HEADER = os.path.join(OWN, "ngp_meshchart.h")
ENTRY_POINTS = ("abi_version", "build_arch", "classify_workspace_bytes", "classify", "label_workspace_bytes", "label", "bounds", "pack",
                "raster", "evict", "dilate", "corners", "texel_points", "render_workspace_bytes", "render")
KERNELS = (b"chart_class", b"vf_count", b"vf_scan", b"vf_fill", b"label_init", b"label_union", b"label_scan", b"label_assign",
           b"chart_bounds", b"chart_raster", b"chart_overlap", b"chart_clear", b"chart_count", b"chart_dilate", b"chart_corners",
           b"chart_points", b"chart_keys", b"chart_shade")
F = np.float32


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


def scenes():
    """name -> (vertices, faces, texel_size): the scenes the issue names, and small sheets."""
    out = {"box": CR.box12() + (1 / 64,), "helicoid": CR.helicoid() + (1 / 64,), "book": CR.book() + (1 / 64,)}
    for level, s in ((2, 1 / 64), (3, 1 / 128)):
        v, f = NR.icosphere(level)[:2]
        out["icosphere%d" % level] = ((np.asarray(v, F) * F(0.4)).astype(F), np.asarray(f, np.int32), s)
    for n in (3, 65, 257):
        out["sheet%d" % n] = CR.sheet(n) + (1 / 64,)
    return out


_CHARTS = {}


def charts_of(name, pad=2):
    if (name, pad) not in _CHARTS:
        v, f, s = scenes()[name]
        _CHARTS[name, pad] = CR.Charts(v, f, s, pad)
    return _CHARTS[name, pad]


# ---- 1. the C ABI


def test_header_compiles_as_c99_alone_and_beside_the_others():
    include = os.path.join(ROOT, "include")
    others = tuple(sorted(n for n in os.listdir(include) if n.endswith(".h")))
    beside = ("ngp_meshatlas.h", "ngp_meshphoto.h", "ngp_meshnormal.h")
    dirs = [os.path.join(ROOT, "ngp_pl_amd", "csrc", d) for d in ("meshchart", "meshatlas", "meshphoto", "meshnormal")]
    inc = lambda names: "".join('#include "%s"\n' % n for n in names)
    for src in ('#include "ngp_meshchart.h"\nint main(void) { return 0; }\n',
                inc(others + beside + ("ngp_meshchart.h",)) + "int main(void) { return NGP_EINVAL + NGP_ERANGE + NGP_MESHCHART_NO_CLASS; }\n",
                inc(("ngp_meshchart.h",) + beside[::-1] + others[::-1]) + "int main(void) { return NGP_EINVAL + NGP_MESHCHART_MAX_PAD; }\n"):
        cmd = ["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", include]
        for d in dirs:
            cmd += ["-I", d]
        r = subprocess.run(cmd + ["-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}
    assert "#ifndef NGP_EINVAL" in text and "#ifndef NGP_ERANGE" in text and "THE RULE" in text
    from ngp_pl_amd import _meshchart_lib
    assert "#define NGP_MESHCHART_NO_CLASS %d" % CR.NO_CLASS in text and _meshchart_lib.NO_CLASS == CR.NO_CLASS
    assert "#define NGP_MESHCHART_MAX_PAD %d" % _meshchart_lib.MAX_PAD in text


def test_library_exports_exactly_its_header_and_no_symbol_of_another_library():
    from ngp_pl_amd import _abi, _meshchart_lib
    protos = _abi.parse(HEADER)
    assert set(protos) == {"ngp_meshchart_" + n for n in ENTRY_POINTS}
    own = _exports(_meshchart_lib.LIB_PATH)
    assert own == set(protos) == set(_meshchart_lib.exported_symbols())
    lib = _meshchart_lib.lib()
    assert lib.ngp_meshchart_abi_version() == 1 == _meshchart_lib.ABI_VERSION and lib.ngp_meshchart_build_arch() == b"gfx950"
    csrc = os.path.dirname(_meshchart_lib.LIB_PATH)
    others = [os.path.join(csrc, n) for n in os.listdir(csrc) if n.startswith("libngp_") and n.endswith(".so") and n != "libngp_meshchart.so"]
    assert len(others) >= 15
    for path in others:
        theirs = _exports(path)
        assert theirs and not theirs & own and not [s for s in theirs if s.startswith("ngp_meshchart")], path


def test_ctypes_agrees_with_the_header():
    from ngp_pl_amd import _abi, _meshchart_lib
    protos = _abi.parse(HEADER)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _meshchart_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    lib = _meshchart_lib.lib()
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        want = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret]
        assert f.restype is want, name


def test_code_object_is_gfx950_only_and_the_build_has_contraction_off():
    from ngp_pl_amd import _meshchart_lib, build
    blob = open(_meshchart_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob
    for kernel in KERNELS:
        assert kernel in blob, kernel
    assert build.MESHCHART_LIB == _meshchart_lib.LIB_PATH and build.MESHCHART_CFLAGS == ["-ffp-contract=off"]
    assert build.ARCH == "gfx950" and build.MESHCHART_SOURCES == [os.path.join("meshchart", "meshchart.hip")]
    for rel in build.MESHCHART_SOURCES + build.MESHCHART_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, rel)), rel
    source = open(os.path.join(build.CSRC, build.MESHCHART_SOURCES[0])).read()
    assert set(re.findall(r'#include\s*"([^"]+)"', source)) == {"ngp_meshchart.h", "../mesh_camera.h", "../mesh_raster.h", "../mesh_host.h",
                                                                 "../mesh_scan.h"}
    assert set(os.path.basename(h) for h in build.MESHCHART_HEADERS) == {"ngp_meshchart.h", "mesh_camera.h", "mesh_raster.h", "mesh_host.h",
                                                                         "mesh_scan.h"}


# ---- 2. the host packer


def _pack(sizes, sort=1, width=0, y0=0):
    from ngp_pl_amd import _meshchart_lib
    sizes = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))
    n = len(sizes)
    origins, order = np.full((n, 2), -7, np.int32), np.full(n, -7, np.int32)
    w, h = C.c_int(-7), C.c_int(-7)
    rc = _meshchart_lib.lib().ngp_meshchart_pack(sizes.ctypes.data, n, sort, width, y0, origins.ctypes.data, order.ctypes.data, C.byref(w),
                                                 C.byref(h))
    return rc, origins.tolist(), order.tolist(), (w.value, h.value)


def test_pack_hand_answers():
    # one chart: W0 = max(10, ceil(sqrt(70)) = 9) = 10, and H(10) = 7
    assert _pack([(10, 7)]) == (0, [[0, 0]], [0], (10, 7))
    # equal heights: four of 5 x 5, area 100, W0 = 10: two shelves of two
    assert _pack([(5, 5)] * 4) == (0, [[0, 0], [5, 0], [0, 5], [5, 5]], [0, 1, 2, 3], (10, 10))
    # a chart exactly W wide: the three higher ones fill the first shelf to x = 12 = W, the wide one opens the second
    assert _pack([(12, 3), (4, 4), (4, 4), (4, 4)]) == (0, [[0, 4], [0, 0], [4, 0], [8, 0]], [1, 2, 3, 0], (12, 7))
    # the width grows: three of 6 x 6, W0 = ceil(sqrt(108)) = 11 holds one per shelf (H = 18 > 11); 11 + max(1, 11 >> 4) = 12 holds two
    assert _pack([(6, 6)] * 3) == (0, [[0, 0], [6, 0], [0, 6]], [0, 1, 2], (12, 12))
    # order: height, then width, then index; unsorted: index
    assert _pack([(2, 3), (5, 3), (2, 9), (5, 3)])[2] == [2, 1, 3, 0] and _pack([(2, 3), (5, 3), (2, 9), (5, 3)], sort=0)[2] == [0, 1, 2, 3]
    # a later stage continues below, at the same width
    assert _pack([(7, 2), (7, 5)], sort=1, width=12, y0=30) == (0, [[0, 35], [0, 30]], [1, 0], (12, 37))
    assert _pack([(7, 2), (7, 5)], sort=0, width=14, y0=30) == (0, [[0, 30], [7, 30]], [0, 1], (14, 35))
    # the limits
    assert _pack([(16384, 16384)])[0] == 0 and _pack([(16384, 16384)])[3] == (16384, 16384)
    untouched = ([[-7, -7]] * 2, (-7, -7))
    for sizes, kw in (([(16384, 16384), (1, 1)], {}), ([(16384, 9000)] * 2, {}), ([(10, 5), (3, 3)], dict(width=100, y0=16380))):
        rc, origins, _, wh = _pack(sizes, **kw)
        assert rc == -5 and (origins, wh) == untouched
        with pytest.raises(ValueError):
            CR.pack(sizes, True, kw.get("width", 0), kw.get("y0", 0))
    for sizes, kw in (([(0, 5)], {}), ([(5, 0)], {}), ([(16385, 1)], {}), ([(1, -1)], {}), ([(5, 5)], dict(width=-1)), ([(5, 5)], dict(width=16385)),
                      ([(5, 5)], dict(y0=3)), ([(5, 5)], dict(width=10, y0=-1)), ([(5, 5)], dict(width=10, y0=16385)), ([(11, 5)], dict(width=10))):
        assert _pack(sizes, **kw)[0] == -1, (sizes, kw)
    from ngp_pl_amd import _meshchart_lib
    lib, x = _meshchart_lib.lib(), C.c_int()
    ok = np.asarray([[3, 3]], np.int32)
    out, order = np.zeros((1, 2), np.int32), np.zeros(1, np.int32)
    full = [ok.ctypes.data, 1, 1, 0, 0, out.ctypes.data, order.ctypes.data, C.byref(x), C.byref(x)]
    assert lib.ngp_meshchart_pack(*full) == 0
    for k in (0, 5, 6, 7, 8):
        args = list(full)
        args[k] = None
        assert lib.ngp_meshchart_pack(*args) == -1, k
    assert lib.ngp_meshchart_pack(*(full[:1] + [0] + full[2:])) == -1 and lib.ngp_meshchart_pack(*(full[:1] + [2 ** 31] + full[2:])) == -5


def test_pack_against_the_restatement():
    g = np.random.RandomState(3)
    for case in range(120):
        n = int(g.randint(1, 60))
        top = int(10 ** g.uniform(0.3, 2.7))
        sizes = g.randint(1, top + 1, (n, 2))
        if case % 3 == 0:
            sizes[:, 1] = sizes[0, 1]                    # equal heights: the order falls to width and index
        for sort in (1, 0):
            origins, order, W, H = CR.pack(sizes, bool(sort))
            assert _pack(sizes, sort) == (0, origins.tolist(), order.tolist(), (W, H)), (case, sort)
            assert H <= W and (origins[:, 0] + sizes[:, 0] <= W).all() and (origins[:, 1] + sizes[:, 1] <= H).all()
            # a later stage below, at that width
            later = np.minimum(g.randint(1, top + 1, (int(g.randint(1, 20)), 2)), [W, 10 ** 6])
            o2, order2, W2, H2 = CR.pack(later, bool(sort), W, H)
            assert W2 == W and _pack(later, sort, W, H) == (0, o2.tolist(), order2.tolist(), (W, H2)) and (o2[:, 1] >= H).all()
            # no two rectangles of the two stages meet
            x0 = np.concatenate([origins[:, 0], o2[:, 0]])
            y0 = np.concatenate([origins[:, 1], o2[:, 1]])
            x1 = x0 + np.concatenate([sizes[:, 0], later[:, 0]])
            y1 = y0 + np.concatenate([sizes[:, 1], later[:, 1]])
            meet = (x0[:, None] < x1[None]) & (x0[None] < x1[:, None]) & (y0[:, None] < y1[None]) & (y0[None] < y1[:, None])
            assert meet.sum() == len(x0)


# ---- 3. host refusals, no GPU


def test_argument_validation_needs_no_gpu():
    from ngp_pl_amd import _lib, _meshchart_lib
    lib = _meshchart_lib.lib()
    V, NF, NCH, AW, AH = 1000, 1800, 7, 90, 80
    W, H, NCAM = 80, 60, 3
    assert lib.ngp_meshchart_render_workspace_bytes(W, H, NCAM) == 8 * W * H * NCAM
    for w, h, n in ((0, H, NCAM), (W, 0, NCAM), (-1, H, NCAM), (16385, H, NCAM), (W, 16385, NCAM), (W, H, 0), (W, H, -1), (W, H, 2 ** 31)):
        assert lib.ngp_meshchart_render_workspace_bytes(w, h, n) == 0
    cb = lib.ngp_meshchart_classify_workspace_bytes(V, NF)
    lb = lib.ngp_meshchart_label_workspace_bytes(NF)
    assert cb >= 4 * (V + 1) and cb % 256 == 0 and lb >= 12 * NF and lb % 256 == 0 and lib.ngp_meshchart_classify_workspace_bytes(0, 1) > 0
    for v, n in ((-1, NF), (2 ** 31, NF), (V, 0), (V, -1), (V, 2 ** 31)):
        assert lib.ngp_meshchart_classify_workspace_bytes(v, n) == 0
    for n in (0, -1, 2 ** 31):
        assert lib.ngp_meshchart_label_workspace_bytes(n) == 0
    fake = C.c_void_p(4096)          # never dereferenced: every call below is rejected before a launch
    odd = C.c_void_p(4100)
    box_ok = (C.c_float * 6)(-1, -1, -1, 1, 1, 1)
    bg_ok = (C.c_float * 3)(1, 1, 1)
    nan, inf = float("nan"), float("inf")
    big = 2 ** 31

    def classify(vertices=fake, faces=fake, n_v=V, n_f=NF, s=0.01, cls=fake, off=fake, vf=fake, ws=fake, wb=cb):
        return ("ngp_meshchart_classify", vertices, faces, n_v, n_f, s, cls, off, vf, ws, wb, None)

    def label(faces=fake, n_v=V, n_f=NF, cls=fake, active=fake, off=fake, vf=fake, unite=1, base=0, lab=fake, chart=fake, n=fake, ws=fake, wb=lb):
        return ("ngp_meshchart_label", faces, n_v, n_f, cls, active, off, vf, unite, base, lab, chart, n, ws, wb, None)

    def bounds(vertices=fake, faces=fake, n_v=V, n_f=NF, s=0.01, chart=fake, lo=0, hi=NCH, out=fake):
        return ("ngp_meshchart_bounds", vertices, faces, n_v, n_f, s, chart, lo, hi, out, None)

    def placed(name, tail, vertices=fake, faces=fake, n_v=V, n_f=NF, s=0.01, chart=fake, rects=fake, n_c=NCH, lo=0, hi=NCH, pad=2, w=AW, h=AH):
        return (name, vertices, faces, n_v, n_f, s, chart, rects, n_c, lo, hi, pad, w, h) + tail + (None,)

    def raster(owner=fake, **kw):
        return placed("ngp_meshchart_raster", (owner,), **kw)

    def evict(owner=fake, ev=fake, n=fake, **kw):
        return placed("ngp_meshchart_evict", (owner, ev, n), **kw)

    def dilate(owner=fake, scratch=C.c_void_p(8192), w=AW, h=AH, pad=2):
        return ("ngp_meshchart_dilate", owner, scratch, w, h, pad, None)

    def corners(vertices=fake, faces=fake, n_v=V, n_f=NF, s=0.01, chart=fake, rects=fake, n_c=NCH, pad=2, w=AW, h=AH, ct=fake, uv=fake):
        return ("ngp_meshchart_corners", vertices, faces, n_v, n_f, s, chart, rects, n_c, pad, w, h, ct, uv, None)

    def points(vertices=fake, faces=fake, normals=fake, n_v=V, n_f=NF, ct=fake, w=AW, h=AH, tf=fake, box=box_ok, begin=0, count=AW * AH, p=fake,
               d=fake, ok=fake):
        return ("ngp_meshchart_texel_points", vertices, faces, normals, n_v, n_f, ct, w, h, tf, box, begin, count, p, d, ok, None)

    def render(vertices=fake, faces=fake, n_v=V, n_f=NF, ct=fake, texture=fake, aw=AW, ah=AH, K=fake, poses=fake, n_c=NCAM, w=W, h=H, near=0.01,
               bg=bg_ok, ws=fake, wb=8 * W * H, image=fake, ids=fake, depth=fake):
        return ("ngp_meshchart_render", vertices, faces, n_v, n_f, ct, texture, aw, ah, K, poses, n_c, w, h, near, bg, ws, wb, image, ids, depth, None)

    def box(k, x):
        b = [-1, -1, -1, 1, 1, 1]
        b[k] = x
        return (C.c_float * 6)(*b)

    def bg(k, x):
        b = [1, 1, 1]
        b[k] = x
        return (C.c_float * 3)(*b)

    bad = [
        classify(vertices=None), classify(faces=None), classify(cls=None), classify(off=None), classify(vf=None), classify(ws=None),
        classify(n_v=-1), classify(n_f=0), classify(n_f=-1), classify(s=0.0), classify(s=-1.0), classify(s=nan), classify(s=inf),
        classify(wb=cb - 1), classify(wb=0), classify(ws=odd), classify(off=odd),
        label(faces=None), label(cls=None), label(active=None), label(off=None), label(vf=None), label(lab=None), label(chart=None), label(n=None),
        label(ws=None), label(n_v=-1), label(n_f=0), label(base=-1), label(wb=lb - 1), label(ws=odd), label(n=odd), label(off=odd),
        bounds(vertices=None), bounds(faces=None), bounds(chart=None), bounds(out=None), bounds(n_v=-1), bounds(n_f=0), bounds(s=0.0), bounds(s=nan),
        bounds(lo=-1), bounds(lo=3, hi=3), bounds(lo=4, hi=3),
        dilate(owner=None), dilate(scratch=None), dilate(scratch=fake), dilate(w=0), dilate(h=0), dilate(w=16385), dilate(h=16385), dilate(pad=-1),
        dilate(pad=9),
        corners(ct=None), corners(uv=None),
        points(vertices=None), points(faces=None), points(normals=None), points(ct=None), points(tf=None), points(box=None), points(p=None),
        points(d=None), points(ok=None), points(n_v=-1), points(n_f=0), points(w=0), points(h=0), points(w=16385), points(h=16385),
        points(begin=-1), points(count=-1), points(begin=1), points(count=AW * AH + 1), points(begin=AW * AH + 1, count=0),
        points(begin=AW * AH, count=1), points(begin=2 ** 62, count=2 ** 62),
        points(box=box(0, nan)), points(box=box(4, nan)), points(box=box(2, -inf)), points(box=box(5, inf)), points(box=box(1, 2.0)),
        render(vertices=None), render(faces=None), render(ct=None), render(texture=None), render(K=None), render(poses=None), render(bg=None),
        render(ws=None), render(image=None), render(n_v=-1), render(n_f=0), render(n_f=-1), render(aw=0), render(ah=0), render(aw=16385),
        render(ah=16385), render(n_c=0), render(n_c=-1), render(w=0), render(h=0), render(w=-1), render(w=16385), render(h=16385),
        render(wb=8 * W * H - 1), render(wb=0), render(ws=odd),
        render(near=nan), render(near=inf), render(near=-inf), render(bg=bg(0, nan)), render(bg=bg(1, inf)), render(bg=bg(2, -inf)),
        raster(owner=None), evict(owner=None), evict(ev=None), evict(n=None), evict(n=odd),
    ]
    for entry in (raster, evict, corners):                # the arguments the placed-face entry points share
        bad += [entry(vertices=None), entry(faces=None), entry(chart=None), entry(rects=None), entry(n_v=-1), entry(n_f=0), entry(n_f=-1),
                entry(s=0.0), entry(s=-2.0), entry(s=nan), entry(s=inf), entry(n_c=0), entry(pad=-1), entry(pad=9), entry(w=0), entry(h=0),
                entry(w=16385), entry(h=16385)]
    for entry in (raster, evict):
        bad += [entry(lo=-1), entry(lo=3, hi=2), entry(hi=NCH + 1)]
    for args in bad:
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshchart_lib.call(*args)
    for args in [classify(n_v=big), classify(n_f=big), label(n_v=big), label(n_f=big), label(base=big - NF), bounds(n_v=big), bounds(n_f=big),
                 bounds(hi=big), raster(n_v=big), raster(n_f=big), raster(n_c=big), evict(n_f=big), corners(n_v=big), corners(n_c=big),
                 points(n_v=big), points(n_f=big), render(n_v=big), render(n_f=big), render(n_c=big)]:
        with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
            _meshchart_lib.call(*args)
    # nothing to do: no launch
    assert _meshchart_lib.call(*points(count=0)) == 0 and _meshchart_lib.call(*points(begin=AW * AH, count=0)) == 0


# ---- 4. the restatement: the scenes' charts and the properties of every atlas


def test_snap_and_class_by_hand():
    s = 1 / 64                                            # c = 1024: a coordinate x snaps to rint(1024 x)
    v = F([[0, 0, 0], [0.25, 0, 0], [0, 0.25, 0], [0, 0, 0.25], [np.nan, 0, 0], [4096.0, 0, 0], [4095.99, 0, 0], [0.0001, 0.0002, 0],
           [1.5 / 1024, 0, 0], [6.5 / 1024, 0, 0], [0, 4.5 / 1024, 0]])
    f = np.int32([[0, 1, 2], [0, 2, 1], [0, 2, 3], [0, 3, 2], [0, 3, 1], [0, 1, 3], [0, 1, 11], [0, -1, 2], [0, 1, 4], [0, 2, 5], [0, 2, 6],
                  [0, 1, 7], [0, 0, 1], [1, 2, 3], [3, 2, 1]])
    cls, X = CR.snap(v, f, s)
    # +z, -z, +x, -x, +y, -y; indices out of range; NaN; 2^22 sixteenths is out, just below is in; a sliver that snaps to a line; a
    # repeated index; a tie of all three components takes the smallest axis
    assert cls.tolist() == [4, 5, 0, 1, 2, 3, 6, 6, 6, 6, 5, 6, 6, 0, 1]
    assert X[0].tolist() == [[0, 0, 0], [256, 0, 0], [0, 256, 0]] and X[6].tolist() == [[0] * 3] * 3 and X[10][2].tolist() == [4194294, 0, 0]
    # halves go to even
    assert CR.snap(v, np.int32([[8, 9, 10]]), s)[1][0].tolist() == [[2, 0, 0], [6, 0, 0], [0, 4, 0]]
    uv = CR.plane(cls, X)
    for k in np.nonzero(cls < 6)[0]:
        (ax, ay), (bx, by), (cx, cy) = uv[k].tolist()
        assert (bx - ax) * (cy - ay) - (by - ay) * (cx - ax) > 0


def test_charts_of_the_scenes():
    for name in ("icosphere2", "icosphere3"):
        c = charts_of(name)
        assert (c.charts_per_stage, c.evicted_per_stage, c.n_charts) == ([6], [0], 6), name
        assert sorted(np.bincount(c.face_class, minlength=7).tolist()[:6]) == sorted(np.bincount(c.face_chart).tolist())
    c = charts_of("box")
    assert c.charts_per_stage == [6] and c.evicted_per_stage == [0] and np.bincount(c.face_chart).tolist() == [2] * 6
    assert c.face_class.tolist() == [1, 1, 0, 0, 3, 3, 2, 2, 5, 5, 4, 4] and c.labels[0].tolist() == [0, 0, 2, 2, 4, 4, 6, 6, 8, 8, 10, 10]
    c = charts_of("helicoid")
    assert c.charts_per_stage == [1, 1, 48] and c.evicted_per_stage == [96, 48] and c.n_charts == 50
    assert (c.face_chart[:48] == 0).all() and (c.face_chart[48:96] == 1).all() and c.face_chart[96:].tolist() == list(range(2, 50))
    c = charts_of("book")                                 # three faces on one edge: the two of one class are one chart
    assert c.face_class.tolist() == [4, 4, 0, 4] and c.labels[0].tolist() == [0, 0, 2, 0] and c.face_chart.tolist() == [0, 0, 1, 0]
    c = charts_of("sheet257")
    assert len(set(c.face_class.tolist())) >= 3 and c.charts_per_stage[0] >= 3


@pytest.mark.parametrize("name,pad", [("box", 2), ("box", 0), ("helicoid", 2), ("helicoid", 8), ("icosphere2", 2), ("icosphere3", 2), ("book", 2),
                                      ("sheet3", 2), ("sheet65", 0), ("sheet257", 2), ("sheet257", 8)])
def test_properties_of_the_atlas(name, pad):
    c = charts_of(name, pad)
    W, H, r = c.W, c.H, c.chart_rects
    # rectangles are disjoint and inside the atlas
    x0, y0, x1, y1 = r[:, 0], r[:, 1], r[:, 0] + r[:, 2], r[:, 1] + r[:, 3]
    assert (x0 >= 0).all() and (y0 >= 0).all() and (x1 <= W).all() and (y1 <= H).all() and W <= 16384 and H <= 16384
    meet = (x0[:, None] < x1[None]) & (x0[None] < x1[:, None]) & (y0[:, None] < y1[None]) & (y0[None] < y1[:, None])
    assert meet.sum() == len(r)
    # no texel centre is covered by two faces that kept the same chart, and every covered centre is owned by the face that covers it
    owner = c.owner.reshape(-1)
    for chart in range(c.n_charts):
        members = np.nonzero(c.face_chart == chart)[0]
        cover = [CR.covered(c.corner_texels[f], W, H) for f in members]
        every = np.concatenate(cover) if cover else np.zeros(0, np.int64)
        assert len(every) == len(np.unique(every)), chart
        for f, t in zip(members, cover):
            assert (owner[t] == f).all()
            xs, ys = t % W, t // W
            assert ((xs >= x0[chart] + pad) & (xs < x1[chart] - pad) & (ys >= y0[chart] + pad) & (ys < y1[chart] - pad)).all()
    owned = c.owner != CR.NO_OWNER
    assert owned.sum() == sum(len(CR.covered(c.corner_texels[f], W, H)) for f in np.nonzero(c.face_chart >= 0)[0])
    # every texel within Chebyshev distance pad of an owned one is filled, by a face of the same rectangle; nothing further is
    near = owned.copy()
    for _ in range(pad):
        grown = near.copy()
        for dx, dy in CR.NEIGHBOURS:
            grown[max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] |= near[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
        near = grown
    assert np.array_equal(c.texel_face >= 0, near)
    assert np.array_equal(c.texel_face[owned], c.owner[owned].astype(np.int32))
    ys, xs = np.nonzero(near)
    ch = c.face_chart[c.texel_face[ys, xs]]
    assert ((xs >= x0[ch]) & (xs < x1[ch]) & (ys >= y0[ch]) & (ys < y1[ch])).all()
    # inside a chart a vertex has one UV
    v, f, _ = scenes()[name]
    seen = {}
    for face in np.nonzero(c.face_chart >= 0)[0]:
        for k in range(3):
            key = (int(c.face_chart[face]), int(f[face, k]))
            assert seen.setdefault(key, tuple(c.corner_texels[face, k])) == tuple(c.corner_texels[face, k])


def test_affine_colour_on_the_box_within_half_a_step():
    """Each chart of the box is flat, the texel points are affine in the texel centre and the border extrapolates the face's plane
    (here the plane of the whole chart), so a colour that is affine in space is affine over every chart's rectangle and the
    bilinear lookup of the exact texel colours is exact, across the faces of a chart too; what is left is the quantisation, half a
    step of 1 / 255 on each of the four texels and so on their convex combination, plus f32 rounding (1e-5)."""
    from tests import mesh_texture_reference as TR
    v, f, s = scenes()["box"]
    c = charts_of("box")
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    p, d, valid = CR.texel_points(v, f, nrm, c, (-1, -1, -1, 1, 1, 1))
    assert np.array_equal(valid.reshape(c.H, c.W) != 0, c.texel_face >= 0)
    texture = TR.quantise(CR.affine_colour(p), valid).reshape(c.H, c.W, 3)
    K, poses, wh = TR.sphere_cameras(3, 48)
    image, ids, depth, beta, gamma = AR.render(v, f, np.zeros((len(f), 2), np.int32), np.zeros((1, 1, 3), np.uint8), K, poses, wh, 0.01,
                                               return_weights=True)
    image = CR.render(v, f, c.corner_texels, texture, K, poses, wh, 0.01)[0]
    covered = ids >= 0
    assert covered.sum() > 0.1 * covered.size
    tri = v.astype(np.float64)[f[ids[covered]]]
    bb, gg = beta[covered].astype(np.float64)[:, None], gamma[covered].astype(np.float64)[:, None]
    hit = tri[:, 0] + bb * (tri[:, 1] - tri[:, 0]) + gg * (tri[:, 2] - tri[:, 0])
    err = np.abs(image[covered].astype(np.float64) - CR.affine_colour(hit)).max()
    print("largest colour error %.6f = %.3f steps of 1/255" % (err, err * 255))
    assert err <= 0.5 / 255 + 1e-5


# ---- 5. GLB


def read_glb(path):
    blob = open(path, "rb").read()
    magic, version, total = struct.unpack("<4sII", blob[:12])
    assert magic == b"glTF" and version == 2 and total == len(blob)
    n, tag = struct.unpack("<I4s", blob[12:20])
    assert tag == b"JSON" and n % 4 == 0
    doc = json.loads(blob[20:20 + n].decode("utf-8"))
    m, tag = struct.unpack("<I4s", blob[20 + n:28 + n])
    assert tag == b"BIN\x00" and m % 4 == 0 and 28 + n + m == len(blob)
    return doc, blob[28 + n:]


def _accessor(doc, binary, k):
    a = doc["accessors"][k]
    view = doc["bufferViews"][a["bufferView"]]
    dtype, width = {5125: ("<u4", 1), 5126: ("<f4", {"SCALAR": 1, "VEC2": 2, "VEC3": 3}[a["type"]])}[a["componentType"]]
    raw = binary[view["byteOffset"]:view["byteOffset"] + view["byteLength"]]
    out = np.frombuffer(raw, dtype).reshape(-1, width)
    assert len(out) == a["count"] and view["byteOffset"] % 4 == 0
    return out


def test_save_glb_round_trip(tmp_path):
    from ngp_pl_amd import mesh
    from tests.test_meshtex_cpu import read_png
    g = np.random.RandomState(5)
    for name in ("box", "helicoid", "sheet65"):
        v, f, s = scenes()[name]
        c = charts_of(name)
        image = g.randint(0, 256, (c.H, c.W, 3)).astype(np.uint8)
        tex = mesh.ChartTexture(s, 2, c.W, c.H, c.n_charts, tuple(c.charts_per_stage), tuple(c.evicted_per_stage), c.face_chart.astype(np.int32),
                                c.chart_rects.astype(np.int32), c.corner_texels.astype(np.int32), c.uvs, c.texel_face, image)
        nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
        for normals in (nrm, None):
            path = str(tmp_path / ("%s%d.glb" % (name, normals is None)))
            mesh.save_glb(path, mesh.Mesh(v, f, normals, None, tex))
            doc, binary = read_glb(path)
            assert doc["asset"]["version"] == "2.0" and doc["buffers"] == [dict(byteLength=len(binary))]
            prim = doc["meshes"][0]["primitives"][0]
            assert set(prim["attributes"]) == ({"POSITION", "TEXCOORD_0", "NORMAL"} if normals is not None else {"POSITION", "TEXCOORD_0"})
            idx = _accessor(doc, binary, prim["indices"]).reshape(-1, 3)
            pos = _accessor(doc, binary, prim["attributes"]["POSITION"])
            uv = _accessor(doc, binary, prim["attributes"]["TEXCOORD_0"])
            # the split vertex count: per chart, the vertices of its faces
            want = sum(len(np.unique(f[c.face_chart == k])) for k in range(c.n_charts))
            assert len(pos) == len(uv) == want and idx.shape == (len(f), 3) and idx.max() == want - 1 and idx.min() == 0
            a = doc["accessors"][prim["attributes"]["POSITION"]]
            assert a["min"] == pos.min(0).tolist() and a["max"] == pos.max(0).tolist()
            assert np.array_equal(pos[idx].view(np.int32), v[f].view(np.int32))
            flipped = np.stack([c.uvs[..., 0], F(1) - c.uvs[..., 1]], -1)
            assert np.array_equal(uv[idx], flipped) and (uv >= 0).all() and (uv <= 1).all()
            if normals is not None:
                assert np.array_equal(_accessor(doc, binary, prim["attributes"]["NORMAL"])[idx], nrm[f])
            view = doc["bufferViews"][doc["images"][0]["bufferView"]]
            png = tmp_path / "inside.png"
            png.write_bytes(binary[view["byteOffset"]:view["byteOffset"] + view["byteLength"]])
            assert doc["images"][0]["mimeType"] == "image/png" and np.array_equal(read_png(str(png)), image)
            mat = doc["materials"][0]
            assert mat["pbrMetallicRoughness"] == dict(baseColorTexture=dict(index=0), metallicFactor=0.0, roughnessFactor=1.0)
            assert "KHR_materials_unlit" in mat["extensions"] and doc["extensionsUsed"] == ["KHR_materials_unlit"]
            assert doc["samplers"][0]["minFilter"] == 9987 and doc["samplers"][0]["magFilter"] == 9729 and doc["textures"] == [dict(sampler=0, source=0)]
    # a per-face atlas gives three vertices per face, and still works
    v, f, s = scenes()["box"]
    a = AR.Atlas(v, f, 0.05)
    image = g.randint(0, 256, (a.H, a.W, 3)).astype(np.uint8)
    tex = mesh.AdaptiveTexture(0.05, 1, 256, a.W, a.H, tuple(a.counts.tolist()), a.order, a.face_place, a.face_texels.astype(np.int32), a.uvs, image)
    path = str(tmp_path / "faces.glb")
    mesh.save_glb(path, mesh.Mesh(v, f, None, None, tex))
    doc, binary = read_glb(path)
    assert doc["accessors"][1]["count"] == 3 * len(f)
    with pytest.raises(ValueError):
        mesh.save_glb(path, mesh.Mesh(v, f, None, None, mesh.dataclasses.replace(tex, image=None)))
    with pytest.raises(ValueError):
        mesh.save_glb(path, mesh.Mesh(v, f, None, None, None))


# ---- 6. the Python API's checks and the CLI


def test_python_api_argument_checks():
    import torch
    from ngp_pl_amd import mesh
    assert [fl.name for fl in mesh.dataclasses.fields(mesh.ChartTexture)] == ["texel_size", "pad", "width", "height", "n_charts", "charts_per_stage",
                                                                             "evicted_per_stage", "face_chart", "chart_rects", "corner_texels",
                                                                             "uvs", "texel_face", "image"]
    v = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    m = mesh.Mesh(v, f, torch.zeros(4, 3))
    box = ((0, 0, 0), (1, 1, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.chart_atlas(m, 0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.texture_atlas(m, texel_size=0.1, charts=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.bake_texture(None, m, texel_size=0.1, charts=dict(pad=3), color_fn=lambda p, d: p, box=box)
    for size in (0, 0.0, -1.0, float("nan"), float("inf"), 1e-60, 1e60, "1", True, (1,), None):
        with pytest.raises(ValueError, match="texel_size"):
            mesh.chart_atlas(m, size)
        with pytest.raises(ValueError):
            mesh.extract_mesh(None, 8, texture=dict(texel_size=size, charts=True))
    for pad in (-1, 9, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="pad"):
            mesh.chart_atlas(m, 0.1, pad)
        with pytest.raises(ValueError, match="pad"):
            mesh.texture_atlas(m, texel_size=0.1, charts=dict(pad=pad))
        with pytest.raises(ValueError, match="pad"):
            mesh.extract_mesh(None, 8, texture=dict(texel_size=1.0, charts=dict(pad=pad)))
    for charts in (1, "yes", dict(border=2), [2]):
        with pytest.raises(ValueError, match="charts"):
            mesh.texture_atlas(m, texel_size=0.1, charts=charts)
    with pytest.raises(ValueError, match="texel_size"):
        mesh.texture_atlas(m, charts=True)
    for kw in (dict(texels=4), dict(min_texels=2), dict(max_texels=64)):
        with pytest.raises(ValueError, match="charts excludes"):
            mesh.texture_atlas(m, texel_size=0.1, charts=True, **kw)
        with pytest.raises(ValueError, match="charts excludes"):
            mesh.bake_texture(None, m, texel_size=0.1, charts=True, color_fn=lambda p, d: p, box=box, **kw)
        with pytest.raises(ValueError, match="charts excludes"):
            mesh.extract_mesh(None, 8, texture=dict(texel_size=1.0, charts=True, **kw))
    for texture in (dict(charts=True), dict(charts=True, max_side=64), dict(texel_size=1.0, charts=True, normal_map=True),
                    dict(texel_size=1.0, charts=True, max_side=64)):
        with pytest.raises(ValueError, match="charts"):
            mesh.extract_mesh(None, 8, texture=texture)
    with pytest.raises(ValueError, match="no faces"):
        mesh.chart_atlas(mesh.Mesh(v, f[:0]), 0.1)
    tex = mesh.ChartTexture(0.1, 2, 4, 4, 1, (1, 0, 0), (0, 0), None, None, None, None, None)
    with pytest.raises(ValueError, match="ChartTexture"):
        mesh.bake_normal_map(mesh.Mesh(v, f, None, None, tex), m, 0.1)
    # charts=None and charts=False are today's calls
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.texture_atlas(m, texel_size=0.1, charts=None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.texture_atlas(m, 4, charts=False)


def test_cli_lists_the_options_and_refuses_bad_combinations(capsys):
    from ngp_pl_amd import mesh
    with pytest.raises(SystemExit) as e:
        mesh.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--texture-charts", "--texture-chart-pad P", ".glb"):
        assert flag in out
    size = ["--texture-texel-size", "1"]
    for bad in (["--out", "y.glb", "--texture-charts"], ["--out", "y.glb", "--texture-chart-pad", "2"] + size,
                ["--out", "y.glb", "--texture-charts", "--texture-chart-pad", "9"] + size,
                ["--out", "y.glb", "--texture-charts", "--texture-chart-pad", "-1"] + size,
                ["--out", "y.glb", "--texture-charts", "--texture-chart-pad", "2.5"] + size,
                ["--out", "y.glb", "--texture-charts", "--texture-max-side", "512"],
                ["--out", "y.obj", "--texture-charts", "--texture-texels", "8"],
                ["--out", "y.obj", "--texture-charts", "--texture-min-texels", "2"] + size,
                ["--out", "y.obj", "--texture-charts", "--texture-max-texels", "64"] + size,
                ["--out", "y.obj", "--texture-charts", "--texture-normal-map", "--simplify-voxels", "2"] + size,
                ["--out", "y.ply", "--texture-charts"] + size, ["--out", "y.glb"],
                ["--out", "y.glb", "--texture-texels", "8", "--texture-normal-map", "--simplify-voxels", "2"]):
        with pytest.raises(SystemExit) as e:
            mesh.main(["--ckpt", "x"] + bad)
        assert e.value.code == 2, bad
        err = capsys.readouterr().err
        assert "--texture-" in err or ".glb" in err or ".obj" in err
