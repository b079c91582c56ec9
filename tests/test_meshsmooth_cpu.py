"""CPU: the C ABI of libngp_meshsmooth.so (header, exports, ctypes, code object, host-side argument checks), the Python API's
argument checks and the CLI's help, and the numpy restatement the GPU tests compare against (tests/mesh_smooth_reference.py): known
answers computed by hand, what the filter does to a noisy sphere (and what a plain Laplacian does instead), an open mesh with its
boundary pinned and free, the order of the faces, and the geometric normals of a sphere."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mc_reference as R
from tests import mesh_smooth_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngp_meshsmooth.h")
OTHERS = ("ngp_hip.h", "ngp_mesh.h", "ngp_meshfilter.h", "ngp_meshcull.h", "ngp_meshsimplify.h", "ngp_meshtsdf.h")
Q = 1 << 16


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


def test_header_compiles_as_c99_alone_and_with_the_other_six_in_any_order():
    inc = lambda names: "".join('#include "%s"\n' % n for n in names)
    for src in ('#include "ngp_meshsmooth.h"\nint main(void) { return 0; }\n',
                inc(OTHERS + ("ngp_meshsmooth.h",)) + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n",
                inc(("ngp_meshsmooth.h",) + OTHERS[::-1]) + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n",
                inc(OTHERS[3:] + ("ngp_meshsmooth.h",) + OTHERS[:3]) + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n"):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}
    assert "#ifndef NGP_EINVAL" in text and "#ifndef NGP_ERANGE" in text


def test_library_exports_exactly_its_header():
    from ngp_pl_amd import _abi, _meshsmooth_lib
    protos = _abi.parse(HEADER)
    assert set(protos) == {"ngp_meshsmooth_" + n for n in ("abi_version", "build_arch", "workspace_bytes", "topology", "taubin", "normals")}
    assert _exports(_meshsmooth_lib.LIB_PATH) == set(protos)
    assert set(_meshsmooth_lib.exported_symbols()) == set(protos)
    lib = _meshsmooth_lib.lib()
    assert lib.ngp_meshsmooth_abi_version() == 1 == _meshsmooth_lib.ABI_VERSION and lib.ngp_meshsmooth_build_arch() == b"gfx950"


def test_the_seven_libraries_share_no_symbol():
    from ngp_pl_amd import _abi, _lib, _mesh_lib, _meshcull_lib, _meshfilter_lib, _meshsimplify_lib, _meshsmooth_lib, _meshtsdf_lib
    mods = (_lib, _mesh_lib, _meshfilter_lib, _meshcull_lib, _meshsimplify_lib, _meshtsdf_lib, _meshsmooth_lib)
    for m in mods:
        m.lib()
    assert len({m.LIB_PATH for m in mods}) == 7
    exports = [_exports(m.LIB_PATH) for m in mods]
    assert all(exports) and len(exports[0]) >= 100
    for i, a in enumerate(exports):
        for b in exports[i + 1:]:
            assert not a & b
    own, others = exports[-1], set().union(*exports[:-1])
    assert not [s for s in others if s.startswith("ngp_meshsmooth")]
    assert not [s for s in own if not s.startswith("ngp_meshsmooth_")]
    declared_elsewhere = set(_abi.parse_all())
    for h in OTHERS[1:]:
        declared_elsewhere |= set(_abi.parse(os.path.join(ROOT, "include", h)))
    assert not set(_abi.parse(HEADER)) & declared_elsewhere


def test_ctypes_agrees_with_the_header():
    from ngp_pl_amd import _abi, _meshsmooth_lib
    protos = _abi.parse(HEADER)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _meshsmooth_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    lib = _meshsmooth_lib.lib()
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        want = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret]
        assert f.restype is want, name


def test_code_object_is_gfx950_only():
    from ngp_pl_amd import _meshsmooth_lib
    blob = open(_meshsmooth_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob


def test_build_links_the_seventh_library_with_contraction_off():
    from ngp_pl_amd import _meshsmooth_lib, build
    assert build.MESHSMOOTH_LIB == _meshsmooth_lib.LIB_PATH and build.MESHSMOOTH_CFLAGS == ["-ffp-contract=off"]
    assert build.ARCH == "gfx950" and all(os.path.exists(os.path.join(build.CSRC, s)) for s in build.MESHSMOOTH_SOURCES)


def test_argument_validation_needs_no_gpu():
    from ngp_pl_amd import _lib, _meshsmooth_lib
    lib = _meshsmooth_lib.lib()
    V, F = 100000, 180000
    ws = lib.ngp_meshsmooth_workspace_bytes(V, F)
    # per vertex: states 32, row offset 8, cursor 4, flags 1, normal sums 24; per face: table 12 B x 2097152 slots, rows 24
    body = (32 + 8 + 4 + 1 + 24) * V + 12 * 2097152 + 24 * F
    assert body <= ws < body + 16 * (V // 2048 + 2) + 16 * 256
    assert 0 < lib.ngp_meshsmooth_workspace_bytes(V, 0) < ws and lib.ngp_meshsmooth_workspace_bytes(0, 0) > 0
    for v, f in ((-1, 5), (5, -1), (2 ** 31, 5), (5, 2 ** 31)):
        assert lib.ngp_meshsmooth_workspace_bytes(v, f) == 0
    assert lib.ngp_meshsmooth_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 1) >= (69 + 24) * (2 ** 31 - 1) + 12 * 2 ** 34     # 64-bit sizes
    fake = C.c_void_p(4096)          # never dereferenced: every call below is rejected before a launch
    big = 2 ** 31

    def topology(vertices=fake, faces=fake, n_v=V, n_f=F, origin=fake, cell=0.5, pin=1, w=fake, wb=ws, degree=fake, flags=fake, totals=fake):
        return ("ngp_meshsmooth_topology", vertices, faces, n_v, n_f, origin, cell, pin, w, wb, degree, flags, totals, None)

    def taubin(vertices=fake, n_v=V, n_f=F, origin=fake, cell=0.5, pairs=10, lam=0.5, mu=-0.53, w=fake, wb=ws, out=fake):
        return ("ngp_meshsmooth_taubin", vertices, n_v, n_f, origin, cell, pairs, lam, mu, w, wb, out, None)

    def normals(vertices=fake, faces=fake, n_v=V, n_f=F, w=fake, wb=ws, out=fake):
        return ("ngp_meshsmooth_normals", vertices, faces, n_v, n_f, w, wb, out, None)

    nan, inf = float("nan"), float("inf")
    bad = [
        topology(vertices=None), topology(faces=None), topology(origin=None), topology(w=None), topology(degree=None), topology(flags=None),
        topology(totals=None), topology(n_v=-1), topology(n_f=-1), topology(wb=0), topology(wb=ws - 1),
        topology(cell=0.0), topology(cell=-1.0), topology(cell=nan), topology(cell=inf), topology(cell=-inf), topology(cell=1e-50),     # 0 as a float
        taubin(vertices=None), taubin(origin=None), taubin(w=None), taubin(out=None), taubin(n_v=-1), taubin(n_f=-1), taubin(wb=ws - 1),
        taubin(cell=0.0), taubin(cell=nan), taubin(cell=inf), taubin(pairs=0), taubin(pairs=-3),
        taubin(lam=nan), taubin(lam=inf), taubin(lam=-inf), taubin(lam=1.0000001), taubin(lam=-1.5),
        taubin(mu=nan), taubin(mu=inf), taubin(mu=-inf), taubin(mu=-1.0000001), taubin(mu=2.0),
        normals(vertices=None), normals(faces=None), normals(w=None), normals(out=None), normals(n_v=-1), normals(n_f=-1), normals(wb=ws - 1),
    ]
    for args in bad:
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshsmooth_lib.call(*args)
    for args in [topology(n_v=big), topology(n_f=big), taubin(n_v=big), taubin(n_f=big), normals(n_v=big), normals(n_f=big)]:
        with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
            _meshsmooth_lib.call(*args)
    # zero vertices: nothing to launch, whatever the faces
    for n_f in (0, 7):
        assert _meshsmooth_lib.call(*topology(vertices=None, faces=None, n_v=0, n_f=n_f, origin=None, w=None, wb=0, degree=None, flags=None,
                                              totals=None)) == 0
        assert _meshsmooth_lib.call(*taubin(vertices=None, n_v=0, n_f=n_f, origin=None, w=None, wb=0, out=None)) == 0
        assert _meshsmooth_lib.call(*normals(vertices=None, faces=None, n_v=0, n_f=n_f, w=None, wb=0, out=None)) == 0


def test_python_api_argument_checks():
    import torch
    from ngp_pl_amd import mesh
    v = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    for fn in (mesh.mesh_topology, mesh.smooth_taubin):
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
        for cell in (0, 0.0, -1.0, float("nan"), float("inf"), 1e-50, 1e39, "x", None):
            with pytest.raises(ValueError):
                fn(mesh.Mesh(v, f), cell)
        for origin in ((0.0, 0.0), (0.0,) * 4, torch.zeros(2), torch.zeros(2, 3)):
            with pytest.raises(ValueError):
                fn(mesh.Mesh(v, f), 0.5, origin=origin)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.smooth_taubin(mesh.Mesh(v, f), 0.5, iterations=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.vertex_normals(mesh.Mesh(v, f))
    with pytest.raises(ValueError):
        mesh.vertex_normals(mesh.Mesh(v, f.long()))
    for it in (-1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="iterations"):
            mesh.smooth_taubin(mesh.Mesh(v, f), 0.5, iterations=it)
    for x in (float("nan"), float("inf"), -float("inf"), 1.5, -1.0000001, "x", None):
        with pytest.raises(ValueError, match="lam"):
            mesh.smooth_taubin(mesh.Mesh(v, f), 0.5, lam=x)
        with pytest.raises(ValueError, match="mu"):
            mesh.smooth_taubin(mesh.Mesh(v, f), 0.5, mu=x)
    for smooth in (-1, 2.5, True, dict(iterations=-1), dict(lam=float("nan")), dict(mu=1.5), dict(iterations=3, passes=2)):
        with pytest.raises(ValueError):
            mesh.extract_mesh(None, 8, smooth=smooth)


def test_cli_help_lists_the_flags(capsys):
    from ngp_pl_amd import mesh
    with pytest.raises(SystemExit) as e:
        mesh.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--smooth-iterations N", "--smooth-lambda L", "--smooth-mu M", "--smooth-free-boundary"):
        assert flag in out
    for bad in (["--smooth-iterations", "-1"], ["--smooth-iterations", "2.5"], ["--smooth-iterations", "3", "--smooth-lambda", "1.5"],
                ["--smooth-iterations", "3", "--smooth-mu", "nan"]):
        with pytest.raises(SystemExit) as e:
            mesh.main(["--ckpt", "x", "--out", "y"] + bad)
        assert e.value.code == 2


# ---- the restatement: known answers


QUAD_V = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]])
QUAD_F = np.int32([[0, 1, 2], [1, 3, 2]])


def test_two_triangles_by_hand():
    o = np.float32([0, 0, 0])
    degree, flags, totals, e = SR.topology(QUAD_V, QUAD_F, o, 1.0, pin_boundary=True)
    assert degree.dtype == np.int32 and flags.dtype == np.uint8 and totals.dtype == np.int64
    assert degree.tolist() == [2, 3, 3, 2] and e.tolist() == [[0, 1], [0, 2], [1, 2], [1, 3], [2, 3]]
    assert flags.tolist() == [3, 3, 3, 3] and totals.tolist() == [5, 4, 0, 4]          # the diagonal occurs twice; every vertex is on the boundary
    assert np.array_equal(SR.taubin(QUAD_V, QUAD_F, o, 1.0, 5, 0.5, -0.53).view(np.int32), QUAD_V.view(np.int32))      # all pinned
    degree, flags, totals, e = SR.topology(QUAD_V, QUAD_F, o, 1.0, pin_boundary=False)
    assert flags.tolist() == [7, 7, 7, 7] and totals.tolist() == [5, 4, 4, 4]
    inside, q = SR.states(QUAD_V, o, 1.0)
    assert inside.all() and q.dtype == np.int64 and q.tolist() == (QUAD_V * Q).astype(int).tolist()
    # vertex 0: neighbours 1, 2: D = (Q, Q, 0), / 2 * 0.5 = Q / 4.  vertex 1: neighbours 0, 2, 3: D = (Q - 3 Q, 2 Q, 0) = (-2 Q, 2 Q, 0),
    # / 3 * 0.5 = -+21845.33 -> -+21845.  vertex 2 mirrors vertex 1, vertex 3 mirrors vertex 0
    q1 = SR.one_pass(q, e, degree, np.ones(4, bool), 0.5)
    assert q1.tolist() == [[16384, 16384, 0], [Q - 21845, 21845, 0], [21845, Q - 21845, 0], [Q - 16384, Q - 16384, 0]]
    got = SR.taubin(QUAD_V, QUAD_F, o, 1.0, 1, 0.5, 0.0, pin_boundary=False)              # mu = 0: the second pass adds rint(0)
    assert got.dtype == np.float32
    assert got.tolist() == [[0.25, 0.25, 0], [43691 / Q, 21845 / Q, 0], [21845 / Q, 43691 / Q, 0], [0.75, 0.75, 0]]
    # a grid that does not start at 0, with a cell that is no power of two: the state is relative to the origin
    inside, q = SR.states(QUAD_V * np.float32(3) + np.float32(7), np.float32([7, 7, 7]), 3.0)
    assert inside.all() and q.tolist() == (QUAD_V * Q).astype(int).tolist()
    # normals of the flat quad: both faces counter-clockwise seen from +z
    assert SR.normals(QUAD_V, QUAD_F).tolist() == [[0, 0, 1]] * 4
    assert SR.normals(QUAD_V, QUAD_F[:, ::-1]).tolist() == [[0, 0, -1]] * 4


def test_states_at_the_edge_of_the_grid_and_rounding():
    nan, inf = np.float32("nan"), np.float32("inf")
    v = np.float32([[16384, 0, 0], [-16384, 0, 0], [16384.002, 0, 0], [0, nan, 0], [0, 0, inf], [0, -inf, 0], [3e38, 0, 0],
                    [0.5 / Q, 1.5 / Q, -0.5 / Q], [2.5 / Q, -1.5 / Q, 0]])
    inside, q = SR.states(v, np.float32([0, 0, 0]), 1.0)
    assert inside.tolist() == [True, True, False, False, False, False, False, True, True]
    assert q[0].tolist() == [SR.QMAX, 0, 0] and q[1].tolist() == [-SR.QMAX, 0, 0] and (q[2:7] == 0).all()
    assert q[7].tolist() == [0, 2, 0] and q[8].tolist() == [2, -2, 0]                    # halves go to the even neighbour
    # ties in a pass: a vertex of degree 1 whose neighbour is an odd number of quanta away, factor 0.5
    v = np.float32([[0, 0, 0], [3 / Q, 1 / Q, -5 / Q], [1, 1, 1]])
    degree, flags, _, e = SR.topology(v, np.int32([[0, 1, 1], [0, 1, 2]]), np.float32([0, 0, 0]), 1.0, False)      # the first face is not valid
    assert degree.tolist() == [2, 2, 2]
    degree, flags, _, e = SR.topology(v, np.int32([[0, 1, 5], [0, 1, -1]]), np.float32([0, 0, 0]), 1.0, False)
    assert degree.tolist() == [0, 0, 0] and flags.tolist() == [1, 1, 1] and len(e) == 0
    trace = {}
    q1 = SR.one_pass(SR.states(v, np.float32([0, 0, 0]), 1.0)[1], np.int64([[0, 1]]), np.int32([1, 1, 0]), np.array([True, True, False]), 0.5, trace)
    assert trace["ties"] == 6 and q1.tolist() == [[2, 0, -2], [1, 1, -3], [Q, Q, Q]]     # 1.5 -> 2, 0.5 -> 0, -2.5 -> -2; 3 - 2, 1 - 0, -5 + 2


def test_the_clamp():
    # two vertices 2^14 cells either side of the origin pushed apart by a negative factor: the state stops at +-QMAX
    v = np.float32([[16000, 0, 0], [-16000, 0, 0], [0, 1, 0]])
    f = np.int32([[0, 1, 2]])
    trace = {}
    out = SR.taubin(v, f, np.float32([0, 0, 0]), 1.0, 1, -1.0, -1.0, pin_boundary=False, trace=trace)
    assert trace["clamped"] > 0 and trace["at_qmax"] > 0
    assert out[0, 0] == 16384 and out[1, 0] == -16384


# ---- the restatement on marching-cubes meshes


def sphere_volume(n, radius):
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, n, dtype=np.float32)] * 3, indexing="ij")
    return (np.float32(radius) - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


@pytest.fixture(scope="module")
def sphere48():
    """Marching cubes of a sphere of radius 0.7 at 48^3; the same with the vertices moved along the radius by up to 0.3 voxel."""
    v, f, n, _ = R.marching_cubes(sphere_volume(48, 0.7), 0.0, (-1, -1, -1), (1, 1, 1))
    h = 2.0 / 47
    r = np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    jitter = np.random.RandomState(0).uniform(-0.3, 0.3, (len(v), 1)) * h
    return v, f, n, (v.astype(np.float64) * (1 + jitter / r)).astype(np.float32), h


def radii(v, h):
    r = np.linalg.norm(v.astype(np.float64), axis=1) / h
    return r.mean(), r.std()


def test_taubin_removes_the_noise_and_keeps_the_size_where_a_laplacian_shrinks(sphere48):
    _, f, _, noisy, h = sphere48
    o, cell = np.float32([-1, -1, -1]), np.float32(h)
    degree, flags, totals, e = SR.topology(noisy, f, o, cell)
    assert totals[1] == 0 and totals[3] == 0 and totals[2] == len(noisy) and totals[0] * 2 == len(f) * 3          # closed and manifold
    print("degrees %d to %d" % (degree.min(), degree.max()))
    mean0, std0 = radii(noisy, h)
    out = SR.taubin(noisy, f, o, cell, 10, 0.5, -0.53)
    assert out.dtype == np.float32 and out.shape == noisy.shape
    mean1, std1 = radii(out, h)
    control = SR.taubin(noisy, f, o, cell, 10, 0.5, 0.5)                                 # mu = +0.5: twenty Laplacian passes
    mean2, std2 = radii(control, h)
    print("mean radius %+.4f voxel, deviation %.4f -> %.4f voxel; Laplacian: mean %+.4f, deviation %.4f" % (mean1 - mean0, std0, std1, mean2 - mean0, std2))
    assert abs(mean1 - mean0) < 0.02 and std1 <= 0.5 * std0
    assert abs(mean2 - mean0) > 0.2 and mean2 < mean0
    # one trip through the grid alone moves a vertex by a quantum and an ulp
    still = SR.taubin(noisy, f, o, cell, 1, 0.0, 0.0)
    assert 0 < np.abs(still.astype(np.float64) - noisy).max() / h < 2e-5


def test_open_mesh_pinned_and_free_boundary(sphere48):
    _, f, _, noisy, h = sphere48
    o, cell = np.float32([-1, -1, -1]), np.float32(h)
    upper = f[(noisy[f][:, :, 2] > 0).all(1)]                                            # the lower half's vertices stay, in no face
    referenced = np.zeros(len(noisy), bool)
    referenced[upper.reshape(-1)] = True
    degree, flags, totals, _ = SR.topology(noisy, upper, o, cell, True)
    boundary, free = (flags & 2) != 0, (flags & 4) != 0
    print("%d boundary vertices, %d of %d referenced vertices free" % (boundary.sum(), free.sum(), referenced.sum()))
    assert 0 < boundary.sum() == totals[3] and totals[1] > 0 and free.sum() == totals[2] == referenced.sum() - boundary.sum()
    assert (degree[~referenced] == 0).all() and (flags[~referenced] == 1).all()
    pinned = SR.taubin(noisy, upper, o, cell, 10, 0.5, -0.53, pin_boundary=True)
    loose = SR.taubin(noisy, upper, o, cell, 10, 0.5, -0.53, pin_boundary=False)
    same = lambda a: (a.view(np.int32) == noisy.view(np.int32)).all(1)
    assert same(pinned)[boundary].all() and not same(pinned)[free].any()
    assert not same(loose)[boundary].any()
    assert same(pinned)[~referenced].all() and same(loose)[~referenced].all()
    flags_loose = SR.topology(noisy, upper, o, cell, False)[1]
    assert ((flags_loose & 4) != 0).sum() == referenced.sum() and np.array_equal(flags_loose & 3, flags & 3)


def test_the_order_of_the_faces_changes_nothing(sphere48):
    _, f, _, noisy, h = sphere48
    o, cell = np.float32([-1, -1, -1]), np.float32(h)
    g = np.random.RandomState(1)
    shuffled = f[g.permutation(len(f))]
    shuffled = np.where((g.randint(0, 2, len(f)) == 1)[:, None], shuffled[:, [1, 2, 0]], shuffled)              # rotated, orientation kept
    for a, b in zip(SR.topology(noisy, f, o, cell), SR.topology(noisy, shuffled, o, cell)):
        assert np.array_equal(a, b)
    assert np.array_equal(SR.taubin(noisy, f, o, cell, 3, 0.5, -0.53).view(np.int32), SR.taubin(noisy, shuffled, o, cell, 3, 0.5, -0.53).view(np.int32))
    assert np.array_equal(SR.normals(noisy, f).view(np.int32), SR.normals(noisy, shuffled).view(np.int32))


def test_geometric_normals_of_a_sphere_are_radial(sphere48):
    v, f, gradient, _, _ = sphere48
    n = SR.normals(v, f)
    assert n.dtype == np.float32 and n.shape == v.shape
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6
    radial = v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)
    cos = (n * radial).sum(1)
    print("min cos to radial %.5f, to the gradient normals %.5f" % (cos.min(), (n * gradient).sum(1).min()))
    assert cos.min() > 0.999
    # degenerate and non-finite faces add nothing; a vertex of no face, or of two faces that cancel, has a zero normal
    nan = np.float32("nan")
    v2 = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [nan, 0, 0], [5, 5, 5], [3e38, 0, 0], [0, 3e38, 0], [7, 7, 7], [8, 7, 7], [7, 8, 7]])
    f2 = np.int32([[8, 9, 10], [8, 10, 9], [0, 1, 3], [0, 1, 1], [0, 1, 4], [0, 1, 11], [-1, 1, 2], [1, 3, 2], [0, 6, 7]])
    n2 = SR.normals(v2, f2)
    assert n2[8:].tolist() == [[0, 0, 0]] * 3                                            # two faces that cancel
    assert n2[4].tolist() == [0, 0, 0] and n2[5].tolist() == [0, 0, 0]                    # a NaN corner; no face
    assert n2[1:4].tolist() == [[0, 0, 1]] * 3                                           # face (1, 3, 2) alone: the others through vertex 1 add nothing
    assert n2[0].tolist() == [0, 0, 1] and n2[6].tolist() == [0, 0, 1]                    # face (0, 6, 7): 9e76 is a double
