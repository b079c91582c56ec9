"""CPU: the C ABI of libngp_meshsimplify.so (header, exports, ctypes, code object, host-side argument checks), the numpy
restatement the GPU tests compare against (tests/mesh_simplify_reference.py) on marching-cubes meshes and on hand-made edge cases
with known answers, the Python API's argument checks and the CLI's help."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mc_reference as R
from tests import mesh_simplify_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngp_meshsimplify.h")
Q = 1 << 20


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


def test_header_compiles_as_c99_alone_and_after_the_other_four():
    for src in ('#include "ngp_meshsimplify.h"\nint main(void) { return 0; }\n',
                '#include "ngp_hip.h"\n#include "ngp_mesh.h"\n#include "ngp_meshfilter.h"\n#include "ngp_meshcull.h"\n'
                '#include "ngp_meshsimplify.h"\nint main(void) { return NGP_EINVAL + NGP_ERANGE; }\n',
                '#include "ngp_meshsimplify.h"\n#include "ngp_meshcull.h"\n#include "ngp_meshfilter.h"\n#include "ngp_mesh.h"\n'
                'int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n'):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}
    assert "#ifndef NGP_EINVAL" in text and "#ifndef NGP_ERANGE" in text


def test_library_exports_exactly_its_header():
    from ngp_pl_amd import _abi, _meshsimplify_lib
    protos = _abi.parse(HEADER)
    assert set(protos) == {"ngp_meshsimplify_" + n for n in ("abi_version", "build_arch", "workspace_bytes", "cluster", "count", "emit")}
    assert _exports(_meshsimplify_lib.LIB_PATH) == set(protos)
    assert set(_meshsimplify_lib.exported_symbols()) == set(protos)
    lib = _meshsimplify_lib.lib()
    assert lib.ngp_meshsimplify_abi_version() == 1 == _meshsimplify_lib.ABI_VERSION and lib.ngp_meshsimplify_build_arch() == b"gfx950"


def test_the_five_libraries_share_no_symbol():
    from ngp_pl_amd import _abi, _lib, _mesh_lib, _meshcull_lib, _meshfilter_lib, _meshsimplify_lib
    mods = (_lib, _mesh_lib, _meshfilter_lib, _meshcull_lib, _meshsimplify_lib)
    for m in mods:
        m.lib()
    exports = [_exports(m.LIB_PATH) for m in mods]
    assert all(exports) and len(exports[0]) >= 100
    for i, a in enumerate(exports):
        for b in exports[i + 1:]:
            assert not a & b
    own, others = exports[-1], set().union(*exports[:-1])
    assert not [s for s in others if s.startswith("ngp_meshsimplify")]
    assert not [s for s in own if not s.startswith("ngp_meshsimplify_")]
    declared_elsewhere = set(_abi.parse_all())
    for h in ("ngp_mesh.h", "ngp_meshfilter.h", "ngp_meshcull.h"):
        declared_elsewhere |= set(_abi.parse(os.path.join(ROOT, "include", h)))
    assert not set(_abi.parse(HEADER)) & declared_elsewhere


def test_ctypes_agrees_with_the_header():
    from ngp_pl_amd import _abi, _meshsimplify_lib
    protos = _abi.parse(HEADER)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _meshsimplify_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    lib = _meshsimplify_lib.lib()
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        want = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret]
        assert f.restype is want, name


def test_code_object_is_gfx950_only():
    from ngp_pl_amd import _meshsimplify_lib
    blob = open(_meshsimplify_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob


def test_argument_validation_needs_no_gpu():
    from ngp_pl_amd import _lib, _meshsimplify_lib
    lib = _meshsimplify_lib.lib()
    V, F = 100000, 180000
    ws = lib.ngp_meshsimplify_workspace_bytes(V, F)
    ws_v = lib.ngp_meshsimplify_workspace_bytes(V, 0)
    # per vertex: table 12 B x 262144 slots, sums 80, attributes 36, compaction 5; per face: triple 12, table 4 B x 524288 slots
    body = 12 * 262144 + (80 + 36 + 5) * V + 12 * F + 4 * 524288
    assert body <= ws < body + 12 * ((V + F) // 2048 + 2) + 16 * 256
    assert 0 < ws_v < ws and lib.ngp_meshsimplify_workspace_bytes(0, 0) > 0
    for v, f in ((-1, 5), (5, -1), (2 ** 31, 5), (5, 2 ** 31)):
        assert lib.ngp_meshsimplify_workspace_bytes(v, f) == 0
    assert lib.ngp_meshsimplify_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1) >= 149 * (2 ** 31 - 1)     # 64-bit sizes: both tables at their 2^31 slots
    fake = C.c_void_p(4096)          # never dereferenced: every call below is rejected before a launch
    big = 2 ** 31

    def cluster(vertices=fake, normals=fake, colors=fake, n_v=V, origin=fake, cell=0.5, w=fake, wb=ws, out=fake):
        return ("ngp_meshsimplify_cluster", vertices, normals, colors, n_v, origin, cell, w, wb, out, None)

    def count(faces=fake, label=fake, n_v=V, n_f=F, w=fake, wb=ws, totals=fake):
        return ("ngp_meshsimplify_count", faces, label, n_v, n_f, w, wb, totals, None)

    def emit(vertices=fake, n_v=V, n_f=F, origin=fake, cell=0.5, w=fake, wb=ws, ov=1, of=1, vo=fake, no=fake, co=fake, fo=fake):
        return ("ngp_meshsimplify_emit", vertices, n_v, n_f, origin, cell, w, wb, ov, of, vo, no, co, fo, None)

    nan, inf = float("nan"), float("inf")
    bad = [
        cluster(vertices=None), cluster(origin=None), cluster(w=None), cluster(out=None), cluster(n_v=-1),
        cluster(cell=0.0), cluster(cell=-1.0), cluster(cell=nan), cluster(cell=inf), cluster(cell=-inf), cluster(cell=1e-50),     # 0 as a float
        cluster(wb=0), cluster(wb=80 * V),
        count(faces=None), count(label=None), count(w=None), count(totals=None), count(wb=ws - 1), count(wb=ws_v), count(n_v=-1), count(n_f=-1),
        emit(vertices=None), emit(origin=None), emit(w=None), emit(wb=ws - 1), emit(vo=None), emit(fo=None), emit(ov=-1), emit(of=-1),
        emit(ov=V + 1), emit(of=F + 1), emit(n_v=-1), emit(n_f=-1), emit(cell=0.0), emit(cell=nan), emit(cell=inf),
    ]
    for args in bad:
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshsimplify_lib.call(*args)
    for args in [cluster(n_v=big), count(n_v=big), count(n_f=big), emit(n_v=big), emit(n_f=big)]:
        with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
            _meshsimplify_lib.call(*args)
    # zero vertices and an empty result: nothing to launch
    assert _meshsimplify_lib.call(*cluster(vertices=None, normals=None, colors=None, n_v=0, origin=None, w=None, wb=0, out=None)) == 0
    assert _meshsimplify_lib.call(*count(faces=None, label=None, n_v=0, n_f=0, w=None, wb=0, totals=None)) == 0
    assert _meshsimplify_lib.call(*count(faces=None, label=None, n_v=0, n_f=7, w=None, wb=0, totals=None)) == 0
    assert _meshsimplify_lib.call(*emit(vertices=None, n_v=0, n_f=0, origin=None, w=None, wb=0, ov=0, of=0, vo=None, no=None, co=None, fo=None)) == 0
    assert _meshsimplify_lib.call(*emit(ov=0, of=0, vo=None, no=None, co=None, fo=None)) == 0


def test_python_api_argument_checks():
    import torch
    from ngp_pl_amd import mesh
    v = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    for fn in (mesh.vertex_clusters, mesh.simplify_clusters):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(mesh.Mesh(v, f), 0.5)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(mesh.Mesh(v, f), 0.5, origin=(0.0, 0.0, 0.0))
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(mesh.Mesh(v[:0], f[:0]), 0.5)
        for bad in (f.long(), f.float(), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(6, dtype=torch.int32), f.numpy()):
            with pytest.raises(ValueError):
                fn(mesh.Mesh(v, bad), 0.5)
        with pytest.raises(ValueError):
            fn(mesh.Mesh(v.double(), f), 0.5)
        with pytest.raises(ValueError):
            fn(mesh.Mesh(v, f, torch.zeros(5, 3)), 0.5)
        with pytest.raises(ValueError):
            fn(mesh.Mesh(v, f, None, torch.zeros(4, 3, dtype=torch.float64)), 0.5)
        for cell in (0, 0.0, -1.0, float("nan"), float("inf"), 1e-50, 1e39, "x", None):
            with pytest.raises(ValueError):
                fn(mesh.Mesh(v, f), cell)
        for origin in ((0.0, 0.0), (0.0,) * 4, torch.zeros(2), torch.zeros(2, 3)):
            with pytest.raises(ValueError):
                fn(mesh.Mesh(v, f), 0.5, origin=origin)
    for k in (0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="simplify_voxels"):
            mesh.extract_mesh(None, 8, simplify_voxels=k)


def test_cli_help_lists_the_flag(capsys):
    from ngp_pl_amd import mesh
    with pytest.raises(SystemExit) as e:
        mesh.main(["--help"])
    assert e.value.code == 0
    assert "--simplify-voxels K" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        mesh.main(["--ckpt", "x", "--out", "y", "--simplify-voxels", "0"])
    assert e.value.code == 2


# ---- the restatement on marching-cubes meshes


def sphere(n):
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, n, dtype=np.float32)] * 3, indexing="ij")
    return (np.float32(0.8) - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


def torus(n):
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, n, dtype=np.float32)] * 3, indexing="ij")
    return (np.float32(0.25) - np.sqrt((np.sqrt(x * x + y * y) - np.float32(0.6)) ** 2 + z * z)).astype(np.float32)


@pytest.fixture(scope="module", params=[("sphere", 24), ("torus", 32)])
def mc_mesh(request):
    name, n = request.param
    v, f, nrm, _ = R.marching_cubes({"sphere": sphere, "torus": torus}[name](n), 0.0, (-1, -1, -1), (1, 1, 1))
    col = (0.5 * (v + 1)).astype(np.float32)
    return v, f, nrm, col, 2.0 / (n - 1)


@pytest.mark.parametrize("K", [2, 3])
def test_restatement_on_marching_cubes_meshes(mc_mesh, K):
    v, f, nrm, col, h = mc_mesh
    origin, cell = np.float32([-1, -1, -1]), np.float32(K * h)
    v1, f1, n1, c1, label, clusters = SR.simplify(v, f, origin, cell, nrm, col)
    assert v1.dtype == n1.dtype == c1.dtype == np.float32 and f1.dtype == label.dtype == np.int32
    assert 0 < len(v1) < len(v) and 0 < len(f1) < len(f) and len(v1) <= clusters < len(v)
    assert np.array_equal(label, SR.vertex_labels(v, origin, cell)) and (label >= 0).all() and (label <= np.arange(len(v))).all()
    assert (label[label] == label).all() and clusters == len(np.unique(label))
    # V' = the distinct labels the surviving faces reference, in ascending order
    lab = label[f]
    ok = (lab[:, 0] != lab[:, 1]) & (lab[:, 1] != lab[:, 2]) & (lab[:, 0] != lab[:, 2])
    used = np.unique(lab[ok])
    assert len(v1) == len(used) and f1.min() == 0 and f1.max() == len(v1) - 1 and len(np.unique(f1)) == len(v1)
    # no degenerate face, no two faces on one vertex set, the faces in input order
    assert (f1[:, 0] != f1[:, 1]).all() and (f1[:, 1] != f1[:, 2]).all() and (f1[:, 0] != f1[:, 2]).all()
    assert len(np.unique(np.sort(f1, 1), axis=0)) == len(f1)
    first = {}
    for i in np.nonzero(ok)[0].tolist():
        first.setdefault(tuple(sorted(lab[i].tolist())), i)
    assert np.array_equal(used[f1], lab[sorted(first.values())])
    # every output vertex inside its cluster's cell (closed: a mean of fractions can round up to the far face)
    _, c, _, _ = SR.cells(v, origin, cell)
    lo = origin.astype(np.float64) + c[used] * np.float64(cell)
    tol = 2.0 ** -23 * 2                                                       # one f32 ulp of a coordinate of magnitude <= 2
    assert (v1 >= lo - tol).all() and (v1 <= lo + np.float64(cell) + tol).all()
    # unit normals (the sphere's and the torus's never cancel within two or three voxels), colours inside the members' range
    assert np.allclose(np.linalg.norm(n1.astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert (c1 >= 0).all() and (c1 <= 1).all() and np.abs(c1 - 0.5 * (v1 + 1)).max() < 2e-6


def test_restatement_with_a_cell_below_the_vertex_spacing(mc_mesh):
    v, f, nrm, col, h = mc_mesh
    d = np.abs(v[:, None, :].astype(np.float64) - v[None, :, :]).max(2)
    np.fill_diagonal(d, np.inf)
    cell = np.float32(d.min() / 2)                       # no two vertices within `cell` on every axis: no cell holds two
    assert cell > 1e-5
    origin = np.float32([-1, -1, -1])
    v1, f1, n1, c1, label, clusters = SR.simplify(v, f, origin, cell, nrm, col)
    assert np.array_equal(label, np.arange(len(v))) and clusters == len(v)
    assert np.array_equal(f1, f) and len(v1) == len(v)
    # positions move by at most cell / Q plus one ulp of the largest x - origin (below 2: 2^-23)
    moved = np.abs(v1.astype(np.float64) - v).max()
    print("moved %.3e, bound %.3e" % (moved, float(cell) / Q + 2.0 ** -23))
    assert moved <= float(cell) / Q + 2.0 ** -23
    assert np.abs(n1.astype(np.float64) - nrm).max() < 2.0 / Q and np.abs(c1.astype(np.float64) - col).max() <= 0.5 / Q + 2.0 ** -25


# ---- hand-made cases with known answers


def simplify(v, f, cell=1.0, origin=(0, 0, 0), normals=None, colors=None):
    return SR.simplify(np.array(v, np.float32), np.array(f, np.int32).reshape(-1, 3), np.float32(origin), np.float32(cell), normals, colors)


def test_duplicates_in_rotated_and_reversed_order_keep_the_lowest_index_and_its_orientation():
    v = [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.25, 0.25, 0.25], [1.25, 0.75, 0.5], [0.5, 0.5, 2.5]]
    # vertices 0 and 3 share cell (0,0,0), 1 and 4 cell (1,0,0)
    f = [[4, 2, 3], [0, 1, 2], [2, 0, 1], [1, 0, 2], [0, 1, 5], [5, 4, 3]]
    v1, f1, _, _, label, clusters = simplify(v, f)
    assert label.tolist() == [0, 1, 2, 0, 1, 5] and clusters == 4
    # face 0 is (label 1, 2, 0): kept with its own orientation; faces 1-3 are the same set; face 4 is new; face 5 repeats face 4 reversed
    assert f1.tolist() == [[1, 2, 0], [0, 1, 3]]
    assert v1.tolist() == [[0.375, 0.375, 0.375], [1.375, 0.625, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 2.5]]


def test_a_face_with_two_corners_in_one_cell_is_dropped():
    v = [[0.1, 0.1, 0.1], [0.9, 0.9, 0.9], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]]
    v1, f1, _, _, label, _ = simplify(v, [[0, 1, 2], [0, 2, 3], [2, 3, 3]])
    assert label.tolist() == [0, 0, 2, 3] and f1.tolist() == [[0, 1, 2]]
    assert v1.tolist() == [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]]
    none = simplify(v, [[0, 1, 2]])
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3) and none[5] == 3


def test_vertices_outside_the_grid_and_face_indices_out_of_range():
    nan, inf = float("nan"), float("inf")
    v = [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [nan, 0.5, 0.5], [0.5, inf, 0.5], [0.5, 0.5, -0.001], [2097152.0, 0.5, 0.5],
         [2097151.0, 0.5, 0.5], [0.5, 0.5, 1.5]]
    f = [[0, 1, 3], [0, 1, 4], [0, 1, 5], [0, 1, 6], [0, 1, 7], [0, 1, -1], [0, 1, 9], [9, 1, 0], [0, 2, 8], [2 ** 31 - 1, 0, 1], [-2 ** 31, 0, 1]]
    nrm = np.array([[0, 0, 1]] * 9, np.float32)
    v1, f1, n1, _, label, clusters = simplify(v, f, normals=nrm)
    assert label.tolist() == [0, 1, 2, -1, -1, -1, -1, 7, 8] and clusters == 5
    assert f1.tolist() == [[0, 1, 3], [0, 2, 4]]          # faces 4 and 8; output vertices are labels 0, 1, 2, 7, 8
    assert v1.tolist() == [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [2097151.0, 0.5, 0.5], [0.5, 0.5, 1.5]]
    assert n1.tolist() == [[0, 0, 1]] * 5
    # the last cell's key uses the top bit of its 21
    assert SR.cells(np.float32(v), np.float32([0, 0, 0]), np.float32(1))[2][7] == 2097151


def test_a_vertex_on_a_cell_boundary_belongs_to_the_upper_cell():
    v = [[1.0, 0.5, 0.5], [0.99999994, 0.5, 0.5], [1.5, 0.5, 0.5], [0.0, 0.0, 0.0], [-0.0, 0.5, 2.0]]
    inside, c, _, q = SR.cells(np.float32(v), np.float32([0, 0, 0]), np.float32(1))
    assert inside.all() and c.tolist() == [[1, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 2]]
    assert q[0].tolist() == [0, Q // 2, Q // 2] and q[4].tolist() == [0, Q // 2, 0]
    v1, f1, _, _, label, _ = simplify(v, [[0, 1, 4], [2, 3, 4]])
    assert label.tolist() == [0, 1, 0, 1, 4] and f1.tolist() == [[0, 1, 2]]
    assert v1[0].tolist() == [1.25, 0.5, 0.5]


def test_a_fraction_that_rounds_up_to_q():
    # 1 - 2^-24 is a float32; times Q it is Q - 1/16, which rints to Q: the vertex lands on the far face of its own cell
    x = np.float32(1) - np.float32(2.0 ** -24)
    inside, c, _, q = SR.cells(np.float32([[x, 0.5, 0.5]]), np.float32([0, 0, 0]), np.float32(1))
    assert inside[0] and c[0].tolist() == [0, 0, 0] and q[0].tolist() == [Q, Q // 2, Q // 2]
    v1, f1, _, _, label, _ = simplify([[x, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5]], [[0, 1, 2]])
    assert label.tolist() == [0, 1, 2] and v1[0].tolist() == [1.0, 0.5, 0.5]


def test_an_unreferenced_vertex_joins_its_cluster_and_shifts_the_mean():
    v = [[0.25, 0.25, 0.25], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.75, 0.75, 0.25], [5.5, 5.5, 5.5]]
    col = np.array([[1, 0, 0.5], [0, 0, 0], [0, 0, 0], [0, 1, float("nan")], [1, 1, 1]], np.float32)
    nrm = np.array([[1, 0, 0], [0, 0, 1], [0, 0, 1], [-1, 0, 0], [0, 1, 0]], np.float32)
    v1, f1, n1, c1, label, clusters = simplify(v, [[0, 1, 2]], normals=nrm, colors=col)
    assert label.tolist() == [0, 1, 2, 0, 4] and clusters == 4 and f1.tolist() == [[0, 1, 2]]
    assert v1.tolist() == [[0.5, 0.5, 0.25], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5]]       # vertex 3 is in no face and still counts
    assert c1.tolist() == [[0.5, 0.5, 0.25], [0, 0, 0], [0, 0, 0]]                   # the NaN contributes 0 to a sum over 2
    assert n1.tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 1]]                          # opposite normals cancel: all zeros
    # attributes are clamped before they are summed
    _, _, n2, c2, _, _ = simplify(v[:3], [[0, 1, 2]], normals=np.float32([[3, 0, 0], [0, -7, 0], [0, 0, 1]]),
                                  colors=np.float32([[2, -1, 0.5], [0, 0, 0], [float("inf"), -float("inf"), 1]]))
    assert n2.tolist() == [[1, 0, 0], [0, -1, 0], [0, 0, 1]] and c2.tolist() == [[1, 0, 0.5], [0, 0, 0], [1, 0, 1]]
