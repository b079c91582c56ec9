"""CPU: the C ABI of libngp_meshquadric.so (header, exports, ctypes, code object, host-side argument checks), the Python API's and
the CLI's argument checks, and the properties of the numpy restatement the GPU tests compare against
(tests/mesh_quadric_reference.py): orientation and face order leave the sums alone, a planar sheet stays at the mean, and the box,
sphere and wedge cases of tests/test_meshquadric_gpu.py hold.  The mesh generators of both files live here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mc_reference as R
from tests import mesh_quadric_reference as QR
from tests import mesh_simplify_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngp_meshquadric.h")
ENTRY_POINTS = ("abi_version", "build_arch", "workspace_bytes", "accumulate", "sums", "place")


# ---- meshes


def sheet(n_v, n_f, seed, w=37):
    """n_v jittered points of a w-wide sheet of unit spacing and n_f faces (j, j + 1, j + w) over them, indices modulo n_v: the
    generator of tests/test_meshsimplify_gpu.py."""
    g = np.random.RandomState(seed)
    i = np.arange(n_v)
    v = np.stack([i % w, i // w, np.zeros(n_v)], 1) + g.uniform(-0.4, 0.4, (n_v, 3))
    j = np.arange(n_f)
    f = np.stack([j % n_v, (j + 1) % n_v, (j + w) % n_v], 1)
    return v.astype(np.float32), f.astype(np.int32), g


BOX_LO, BOX_HI = np.float64([0.013, 0.021, 0.034]), np.float64([1.013, 1.021, 1.034])
BOX_CASES = [(24, 0.1375), (24, 0.09), (12, 0.29)]


def box(n):
    """The box BOX_LO..BOX_HI: six sides of n x n quads, two triangles each, welded along the edges."""
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        quad.append(vid(tuple(p)))
                    if side == 0:
                        quad.reverse()
                    faces += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    v = BOX_LO[None, :] + np.array(verts, np.float64) / n * (BOX_HI - BOX_LO)[None, :]
    return v.astype(np.float32), np.array(faces, np.int32)


def box_distance(p):
    """Distance of points to the surface of the box BOX_LO..BOX_HI, in float64."""
    p = np.asarray(p, np.float64)
    outside = np.maximum(np.maximum(BOX_LO - p, p - BOX_HI), 0.0)
    d_out = np.sqrt((outside ** 2).sum(1))
    d_in = np.minimum(p - BOX_LO, BOX_HI - p).min(1)
    return np.where(d_out > 0, d_out, d_in)


def wedge(slope, n=9):
    """Two n x n-vertex sheets z = +slope x and z = -slope x over x in [2.55, 3.45], y in [0.1, 0.9]."""
    x, y = np.meshgrid(np.linspace(2.55, 3.45, n), np.linspace(0.1, 0.9, n), indexing="ij")
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).reshape(-1)
    f = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)])
    v = [np.stack([x, y, s * slope * x], -1).reshape(-1, 3) for s in (1, -1)]
    return np.concatenate(v).astype(np.float32), np.concatenate([f, f + n * n]).astype(np.int32)


WEDGE_ORIGIN, WEDGE_CELL = (0.0, 0.0, -0.5), 1.0


def sphere48():
    """The 48^3 marching-cubes sphere of tests/test_meshsimplify_gpu.py: vertices, faces."""
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, 48, dtype=np.float32)] * 3, indexing="ij")
    v, f, _, _ = R.marching_cubes((np.float32(0.8) - np.sqrt(x * x + y * y + z * z)).astype(np.float32), 0.0, (-1, -1, -1), (1, 1, 1))
    return v, f


@pytest.fixture(scope="module")
def sphere():
    return sphere48()


def radial_error(p):
    return np.abs(np.sqrt((np.asarray(p, np.float64) ** 2).sum(1)) - 0.8).mean()


# ---- the C ABI


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


def test_header_compiles_as_c99_alone_and_beside_the_simplifier():
    for src in ('#include "ngp_meshquadric.h"\nint main(void) { return 0; }\n',
                '#include "ngp_meshsimplify.h"\n#include "ngp_meshquadric.h"\nint main(void) { return NGP_EINVAL + NGP_ERANGE; }\n',
                '#include "ngp_meshquadric.h"\n#include "ngp_meshsimplify.h"\n#include "ngp_hip.h"\n'
                'int main(void) { return NGP_EINVAL + NGP_ERANGE + NGP_MESHQUADRIC_SUMS; }\n'):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}
    assert "#ifndef NGP_EINVAL" in text and "#ifndef NGP_ERANGE" in text


def test_library_exports_exactly_its_header():
    from ngp_pl_amd import _abi, _meshquadric_lib
    protos = _abi.parse(HEADER)
    assert set(protos) == {"ngp_meshquadric_" + n for n in ENTRY_POINTS}
    assert _exports(_meshquadric_lib.LIB_PATH) == set(protos)
    assert set(_meshquadric_lib.exported_symbols()) == set(protos)
    lib = _meshquadric_lib.lib()
    assert lib.ngp_meshquadric_abi_version() == 1 == _meshquadric_lib.ABI_VERSION and lib.ngp_meshquadric_build_arch() == b"gfx950"
    text = open(HEADER).read()
    for name in ("SUMS", "NOT_LEADER", "QUADRIC", "MEAN_NO_FACES", "MEAN_OUTSIDE"):
        value = int(re.search(r"#define NGP_MESHQUADRIC_%s\s+(\d+)" % name, text).group(1))
        assert value == getattr(_meshquadric_lib, name) == getattr(QR, name)


def test_no_symbol_shared_with_the_other_libraries():
    from ngp_pl_amd import (_abi, _lib, _mesh_lib, _meshcull_lib, _meshdist_lib, _meshfilter_lib, _meshquadric_lib, _meshsimplify_lib,
                            _meshsmooth_lib, _meshtex_lib, _meshtsdf_lib, _metrics_lib)
    others = (_lib, _mesh_lib, _meshfilter_lib, _meshcull_lib, _meshsimplify_lib, _meshtsdf_lib, _meshsmooth_lib, _meshtex_lib, _metrics_lib,
              _meshdist_lib)
    own = _exports(_meshquadric_lib.LIB_PATH)
    assert own and not [s for s in own if not s.startswith("ngp_meshquadric_")]
    declared = set(_abi.parse(HEADER))
    for m in others:
        theirs = _exports(m.LIB_PATH)
        assert theirs and not own & theirs and not [s for s in theirs if s.startswith("ngp_meshquadric")]
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "ngp_meshquadric.h":
            assert not declared & set(_abi.parse(os.path.join(ROOT, "include", h))), h


def test_ctypes_agrees_with_the_header():
    from ngp_pl_amd import _abi, _meshquadric_lib
    protos = _abi.parse(HEADER)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _meshquadric_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    lib = _meshquadric_lib.lib()
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        want = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret]
        assert f.restype is want, name


def test_code_object_is_gfx950_only():
    from ngp_pl_amd import _meshquadric_lib
    blob = open(_meshquadric_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob


def test_build_entry_compiles_without_contraction():
    from ngp_pl_amd import build
    assert build.MESHQUADRIC_LIB == os.path.join(build.CSRC, "libngp_meshquadric.so")
    assert "-ffp-contract=off" in build.MESHQUADRIC_CFLAGS
    for rel in build.MESHQUADRIC_SOURCES + build.MESHQUADRIC_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, rel)), rel


def test_argument_validation_needs_no_gpu():
    from ngp_pl_amd import _lib, _meshquadric_lib
    lib = _meshquadric_lib.lib()
    V, F = 100000, 180000
    ws = lib.ngp_meshquadric_workspace_bytes(V, F)
    assert 112 * V <= ws < 112 * V + 256 and ws % 256 == 0
    assert lib.ngp_meshquadric_workspace_bytes(V, 0) == ws and lib.ngp_meshquadric_workspace_bytes(0, 0) == 256
    for v, f in ((-1, 5), (5, -1), (2 ** 31, 5), (5, 2 ** 31)):
        assert lib.ngp_meshquadric_workspace_bytes(v, f) == 0
    assert lib.ngp_meshquadric_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1) >= 112 * (2 ** 31 - 1)
    fake = C.c_void_p(4096)          # never dereferenced: every call below is rejected before a launch
    big = 2 ** 31

    def accumulate(vertices=fake, faces=fake, label=fake, n_v=V, n_f=F, origin=fake, cell=0.5, w=fake, wb=ws):
        return ("ngp_meshquadric_accumulate", vertices, faces, label, n_v, n_f, origin, cell, w, wb, None)

    def sums(label=fake, n_v=V, w=fake, wb=ws, out=fake):
        return ("ngp_meshquadric_sums", label, n_v, w, wb, out, None)

    def place(vertices=fake, label=fake, n_v=V, origin=fake, cell=0.5, w=fake, wb=ws, positions=fake, state=fake, totals=fake):
        return ("ngp_meshquadric_place", vertices, label, n_v, origin, cell, w, wb, positions, state, totals, None)

    nan, inf = float("nan"), float("inf")
    bad = [
        accumulate(vertices=None), accumulate(faces=None), accumulate(label=None), accumulate(origin=None), accumulate(w=None),
        accumulate(n_v=-1), accumulate(n_f=-1), accumulate(wb=ws - 1), accumulate(wb=0),
        accumulate(cell=0.0), accumulate(cell=-1.0), accumulate(cell=nan), accumulate(cell=inf), accumulate(cell=-inf), accumulate(cell=1e-50),
        sums(label=None), sums(w=None), sums(out=None), sums(n_v=-1), sums(wb=ws - 1),
        place(vertices=None), place(label=None), place(origin=None), place(w=None), place(positions=None), place(state=None),
        place(totals=None), place(n_v=-1), place(wb=ws - 1), place(cell=0.0), place(cell=nan), place(cell=inf),
    ]
    for args in bad:
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshquadric_lib.call(*args)
    for args in [accumulate(n_v=big), accumulate(n_f=big), sums(n_v=big), place(n_v=big)]:
        with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
            _meshquadric_lib.call(*args)
    # zero vertices: nothing to launch
    assert _meshquadric_lib.call(*accumulate(vertices=None, faces=None, label=None, n_v=0, n_f=0, origin=None, w=None, wb=0)) == 0
    assert _meshquadric_lib.call(*accumulate(vertices=None, faces=None, label=None, n_v=0, n_f=7, origin=None, w=None, wb=0)) == 0
    assert _meshquadric_lib.call(*sums(label=None, n_v=0, w=None, wb=0, out=None)) == 0
    assert _meshquadric_lib.call(*place(vertices=None, label=None, n_v=0, origin=None, w=None, wb=0, positions=None, state=None, totals=None)) == 0


def test_python_api_argument_checks():
    import torch
    from ngp_pl_amd import mesh
    v = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    quadric = lambda m, cell, **kw: mesh.simplify_clusters(m, cell, placement="quadric", **kw)
    for fn in (mesh.cluster_placement, quadric):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(mesh.Mesh(v, f), 0.5)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(mesh.Mesh(v, f), 0.5, origin=(0.0, 0.0, 0.0))
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(mesh.Mesh(v[:0], f[:0]), 0.5)
        for bad in (f.long(), f.float(), torch.zeros(2, 4, dtype=torch.int32), f.numpy()):
            with pytest.raises(ValueError):
                fn(mesh.Mesh(v, bad), 0.5)
        with pytest.raises(ValueError):
            fn(mesh.Mesh(v.double(), f), 0.5)
        for cell in (0, -1.0, float("nan"), float("inf"), 1e-50, 1e39, "x", None):
            with pytest.raises(ValueError):
                fn(mesh.Mesh(v, f), cell)
        for origin in ((0.0, 0.0), (0.0,) * 4, torch.zeros(2)):
            with pytest.raises(ValueError):
                fn(mesh.Mesh(v, f), 0.5, origin=origin)
    for word in ("Quadric", "qem", "", None, 1):
        with pytest.raises(ValueError, match="placement"):
            mesh.simplify_clusters(mesh.Mesh(v, f), 0.5, placement=word)
        with pytest.raises(ValueError, match="simplify_placement"):
            mesh.extract_mesh(None, 8, simplify_voxels=2, simplify_placement=word)
    with pytest.raises(ValueError, match="simplify_placement"):
        mesh.extract_mesh(None, 8, simplify_placement="quadric")               # nothing to place without simplify_voxels


def test_cli_flag(capsys):
    from ngp_pl_amd import mesh
    with pytest.raises(SystemExit) as e:
        mesh.main(["--help"])
    assert e.value.code == 0
    assert re.search(r"--simplify-placement \{mean,quadric\}", capsys.readouterr().out)
    for argv in (["--simplify-placement", "quadric"],                          # without --simplify-voxels
                 ["--simplify-placement", "mean"],
                 ["--simplify-voxels", "2", "--simplify-placement", "median"],
                 ["--simplify-voxels", "2", "--simplify-placement"]):
        with pytest.raises(SystemExit) as e:
            mesh.main(["--ckpt", "x", "--out", "y.ply"] + argv)
        assert e.value.code == 2
        assert "--simplify-placement" in capsys.readouterr().err


# ---- properties of the restatement


def test_orientation_and_face_order_leave_the_sums_alone():
    v, f, g = sheet(900, 1500, 21)
    v[:, 2] += np.float32(0.3) * v[:, 0]                                       # off the grid's axes: no normal is (0, 0, 1)
    origin, cell = np.float32([-1, -1, -2]), np.float32(2.3)
    label = SR.vertex_labels(v, origin, cell)
    s = QR.sums(v, f, label, origin, cell)
    assert s[:, 13].sum() > 0 and (s[:, 4:10] != 0).any(0).all() and (s[:, 10:13] != 0).any(0).all()
    assert np.array_equal(QR.sums(v, f[:, ::-1], label, origin, cell), s)
    assert np.array_equal(QR.sums(v, f[:, [0, 2, 1]], label, origin, cell), s)
    assert np.array_equal(QR.sums(v, f[g.permutation(len(f))], label, origin, cell), s)
    flip = g.rand(len(f)) < 0.5
    mixed = np.where(flip[:, None], f[:, ::-1], f)
    assert np.array_equal(QR.sums(v, mixed[g.permutation(len(f))], label, origin, cell), s)
    # only the labels' own rows are written, and the member sums are the simplifier's
    assert (s[label[label >= 0] != np.arange(len(v))[label >= 0]] == 0).all()
    assert np.array_equal(s[:, 0], np.bincount(label[label >= 0], minlength=len(v)))


def planar_sheet(base, tilted, n=40):
    """An n x n-vertex sheet of half-cell spacing for cell 2^-6 and origin (base, base, base), on the plane z = base + 0.77... or
    z - base = 0.25 (x - base) - 0.5 (y - base) + 0.5.  Every coordinate is a multiple of 2^-12: the vertices are exact in f32 and
    lie on the plane exactly, and so does every cluster's mean."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    g = np.random.RandomState(22)
    x = 0.0625 + (8 * i + g.randint(-1, 2, i.shape)) / 1024.0                  # jitter in steps of 2^-10
    y = 0.0625 + (8 * j + g.randint(-1, 2, i.shape)) / 1024.0
    z = 0.25 * x - 0.5 * y + 0.5 if tilted else np.full(i.shape, 0.7705078125)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)]).astype(np.int32)
    exact = base + np.stack([x, y, z], -1).reshape(-1, 3)
    v = exact.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), exact) and base <= v.min() and v.max() < 2 * base
    return v, f, np.float32([base] * 3), np.float32(2.0 ** -6)


@pytest.mark.parametrize("base,tilted", [(4, False), (512, False), (512, True), (4, True)])
def test_a_planar_sheet_stays_at_the_mean(base, tilted):
    """With one plane the exact minimiser is the mean plus a multiple of the normal, and the mean lies on the plane: it IS the mean.
    What the rule adds is the rounding of the k corner terms of a cluster to integers, at most 1/2 per entry of A and B:
        (M + dA) (y - m) = dB - dA m,   |dB|_2 <= sqrt(3) k/2,   |dA m|_2 <= |dA|_F |m|_2 <= (3 k/2) (sqrt(3)/2)
    and the smallest eigenvalue of M, in the plane, is r = EPS Wsum >= EPS k w S when every corner weighs at least w, against which
    |dA|_2 <= 3k/2 is 3e-3 or less here.  So |y - m| <= 2.17 k / (0.997 r) <= 2.18 / (EPS w S) cells, 2.2e-3 cell for w = 0.06: the
    price of EPS = 2^-10 against S = 2^24.  An axis-aligned plane has n = (0, 0, +-1) exactly, dA and dB vanish in the plane and
    across it B = A m holds exactly: there the two f64 positions agree to rounding.
    Against the final f32 rounding: with coordinates in [512, 1024) an ulp is 2^-14 = 3.9e-3 cell, above the bound, so the two
    results are the same float or neighbours for either plane; in [4, 8) an ulp is 3.1e-5 cell, which the axis-aligned plane meets
    and the tilted one cannot: there the derived bound is asserted instead, and the measured figure printed."""
    v, f, origin, cell = planar_sheet(base, tilted)
    q = QR.simplify(v, f, origin, cell, placement="quadric")
    m = QR.simplify(v, f, origin, cell, placement="mean")
    p = v.astype(np.float64)
    w = 0.5 * np.linalg.norm(np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]), axis=1) / float(cell) ** 2
    assert w.min() >= 0.06                                                     # every corner's weight
    assert (q[6] == QR.QUADRIC).all() and len(q[0]) > 300
    steps = np.abs(q[0].view(np.int32).astype(np.int64) - m[0].view(np.int32)).max()
    moved = np.abs(q[0].astype(np.float64) - m[0]).max() / float(cell)
    bound = 2.18 / (float(QR.EPS) * 0.06 * float(QR.S))
    print("planar sheet base %d tilted %s: worst difference %d ulp, %.3e cell (bound %.3e)" % (base, tilted, steps, moved, bound))
    if base == 4 and tilted:
        assert moved <= bound + 2.0 ** -15
    else:
        assert steps <= 1


@pytest.mark.parametrize("n,cell", BOX_CASES)
def test_box_vertices_land_on_the_surface(n, cell):
    v, f = box(n)
    assert len(v) == (n + 1) ** 3 - (n - 1) ** 3 and len(f) == 12 * n * n
    origin = np.float32([0, 0, 0])
    q = QR.simplify(v, f, origin, np.float32(cell), placement="quadric")
    m = QR.simplify(v, f, origin, np.float32(cell), placement="mean")
    dq, dm = box_distance(q[0]) / cell, box_distance(m[0]) / cell
    print("box n=%d cell=%g: quadric worst %.3e cell, mean worst %.3e cell, %d vertices" % (n, cell, dq.max(), dm.max(), len(q[0])))
    assert np.array_equal(q[1], m[1]) and len(q[0]) == len(m[0]) > 0
    assert dq.max() <= 1.0 / 256
    assert dm.max() >= 1.0 / 8
    _, state, _, _, totals = QR.cluster_placement(v, f, origin, np.float32(cell))
    assert totals[2] == 0 and totals[1] == 0 and (q[6] == QR.QUADRIC).all() and totals[0] == (state == QR.QUADRIC).sum()


@pytest.mark.parametrize("K", [2, 3, 4.5])
def test_sphere_radial_error_drops(sphere, K):
    v, f = sphere
    origin, cell = np.float32([-1, -1, -1]), np.float32(K * 2.0 / 47)
    q = QR.simplify(v, f, origin, cell, placement="quadric")
    m = QR.simplify(v, f, origin, cell, placement="mean")
    eq, em = radial_error(q[0]), radial_error(m[0])
    print("sphere K=%g: quadric %.3e, mean %.3e, %d of %d MEAN_OUTSIDE" % (K, eq, em, (q[6] == QR.MEAN_OUTSIDE).sum(), len(q[6])))
    assert eq < em
    assert (q[6] == QR.MEAN_OUTSIDE).sum() * 8 <= len(q[6])


def test_wedge_falls_back_to_the_mean():
    v, f = wedge(0.1)
    origin, cell = np.float32(WEDGE_ORIGIN), np.float32(WEDGE_CELL)
    positions, state, label, _, totals = QR.cluster_placement(v, f, origin, cell)
    assert sorted(np.unique(label).tolist()) == sorted(np.nonzero(state)[0].tolist()) and totals.tolist() == [0, 0, 2]
    # the simplifier's mean, bit for bit: its expression on the same sums
    inside, c, _, qq = SR.cells(v, origin, cell)
    for lead in np.nonzero(state)[0]:
        members = label == lead
        mean = (qq[members].sum(0).astype(np.float64) / members.sum()) / (1 << 20)
        want = (origin.astype(np.float64) + (c[lead].astype(np.float64) + mean) * np.float64(cell)).astype(np.float32)
        assert np.array_equal(positions[lead].view(np.int32), want.view(np.int32))
    # a shallower wedge: one cluster's crease is within reach, the other's is not
    v, f = wedge(0.02)
    _, state, _, _, totals = QR.cluster_placement(v, f, origin, cell)
    print("wedge 0.02: totals", totals.tolist())
    assert totals[0] >= 1 and totals[2] >= 1 and totals.sum() == 2
