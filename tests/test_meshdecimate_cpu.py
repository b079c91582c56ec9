"""CPU: the C ABI of libngp_meshdecimate.so (header, exports, ctypes, code object, build entry, host-side argument checks), the
Python API's and the CLI's argument checks, and the numpy restatement the GPU tests compare against
(tests/mesh_decimate_reference.py): fans, a boundary, a bow-tie and a tetrahedron by hand, the boxes down to their 8 corners, the
48^3 sphere to the face counts of the clustering, an open cap's boundary, and a permutation of the faces.  The meshes and the
restatement's results that tests/test_meshdecimate_gpu.py compares against are made here, once."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mc_reference as R
from tests import mesh_decimate_reference as DR
from tests import mesh_simplify_reference as SR
from tests import test_meshquadric_cpu as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngp_meshdecimate.h")
ENTRY_POINTS = ("abi_version", "build_arch", "workspace_bytes", "begin", "round", "apply", "count", "emit")
SPHERE_CELL = 2.0 / 47


# ---- meshes and shared results


def fan(n, open_at=None, z=0.0):
    """Vertex 0 at the origin inside a ring 1..n on the plane z: vertex 1 at (0.2, 0), the others on the unit circle; faces
    (0, i, i + 1), without face `open_at` when given."""
    t = 2 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(t), np.sin(t), np.full(n, z)], 1)
    ring[0, 0] = 0.2
    v = np.concatenate([[[0, 0, z]], ring]).astype(np.float32)
    f = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n) if i != open_at], np.int32)
    return v, f


def tetrahedron():
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    return v, np.int32([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])


def big_fan(degree):
    """A closed fan of `degree` faces around vertex 0 on the plane z = 0, inside a second ring of `degree` vertices, so that the
    inner ring's vertices are interior too (5 faces each) and read the centre's row as a target's."""
    t = 2 * np.pi * np.arange(degree) / degree
    inner = np.stack([np.cos(t), np.sin(t), 0 * t], 1)
    outer = 2.0 * np.stack([np.cos(t + np.pi / degree), np.sin(t + np.pi / degree), 0 * t], 1)
    v = np.concatenate([[[0, 0, 0]], inner, outer]).astype(np.float32)
    f = []
    for i in range(degree):
        j = (i + 1) % degree
        f += [[0, 1 + i, 1 + j], [1 + i, 1 + degree + i, 1 + j], [1 + j, 1 + degree + i, 1 + degree + j]]
    return v, np.array(f, np.int32)


@functools.lru_cache(maxsize=None)
def sphere():
    return G.sphere48()


@functools.lru_cache(maxsize=None)
def cluster_faces(K):
    """Vertices and faces of the mean clustering of the sphere with cells of K voxels."""
    v, f = sphere()
    out = SR.simplify(v, f, np.float32([-1, -1, -1]), np.float32(K * SPHERE_CELL))
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def sphere_decimated(K):
    v, f = sphere()
    return DR.decimate(v, f, SPHERE_CELL, target_faces=len(cluster_faces(K)[1]))


@functools.lru_cache(maxsize=None)
def box_decimated(n):
    v, f = G.box(n)
    return DR.decimate(v, f, 1.0 / n, max_error=0.0)


def cap():
    """The faces of the sphere whose three vertices lie above z = 0.3: an open mesh with one boundary loop."""
    v, f = sphere()
    return v, np.ascontiguousarray(f[(v[f][:, :, 2] > 0.3).all(1)])


def surface_error(v, f):
    """| |p| - 0.8 | over face centroids and edge midpoints: mean, max."""
    p = v.astype(np.float64)[f]
    pts = np.concatenate([p.mean(1), (0.5 * (p + p[:, [1, 2, 0]])).reshape(-1, 3)])
    e = np.abs(np.sqrt((pts ** 2).sum(1)) - 0.8)
    return e.mean(), e.max()


def input_index(v_in, v_out):
    """The input index of every output vertex (positions are distinct), ascending when the order is kept."""
    table = {p.tobytes(): i for i, p in enumerate(v_in)}
    return np.array([table[p.tobytes()] for p in v_out], np.int64)


def boundary_edges(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    u, n = np.unique(e, axis=0, return_counts=True)
    return {tuple(x) for x in u[n == 1].tolist()}


# ---- the C ABI


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


def test_header_compiles_as_c99_alone_and_beside_the_others():
    others = sorted(h for h in os.listdir(os.path.join(ROOT, "include")) if h != "ngp_meshdecimate.h")
    assert len(others) == 11
    after = "".join('#include "%s"\n' % h for h in others) + '#include "ngp_meshdecimate.h"\n'
    before = '#include "ngp_meshdecimate.h"\n' + "".join('#include "%s"\n' % h for h in others)
    for src in ('#include "ngp_meshdecimate.h"\nint main(void) { return 0; }\n',
                after + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n",
                before + "int main(void) { return NGP_EINVAL + NGP_ERANGE + NGP_MESHDECIMATE_MAX_DEGREE; }\n"):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}
    assert "#ifndef NGP_EINVAL" in text and "#ifndef NGP_ERANGE" in text


def test_library_exports_exactly_its_header():
    from ngp_pl_amd import _abi, _meshdecimate_lib
    protos = _abi.parse(HEADER)
    assert set(protos) == {"ngp_meshdecimate_" + n for n in ENTRY_POINTS}
    assert _exports(_meshdecimate_lib.LIB_PATH) == set(protos)
    assert set(_meshdecimate_lib.exported_symbols()) == set(protos)
    lib = _meshdecimate_lib.lib()
    assert lib.ngp_meshdecimate_abi_version() == 1 == _meshdecimate_lib.ABI_VERSION and lib.ngp_meshdecimate_build_arch() == b"gfx950"
    text = open(HEADER).read()
    for name in ("MAX_DEGREE", "MAX_FACES"):
        value = int(re.search(r"#define NGP_MESHDECIMATE_%s\s+(\d+)" % name, text).group(1))
        assert value == getattr(_meshdecimate_lib, name)
    assert DR.MAX_DEGREE == _meshdecimate_lib.MAX_DEGREE and _meshdecimate_lib.MAX_FACES == (2 ** 31 - 1) // 3
    # the constants of THE RULE are the restatement's
    assert "S = 1048576 (2^20)" in text and DR.S == 1048576 and "CAP = 1125899906842624 (2^50)" in text and DR.CAP == 2 ** 50
    assert "0x9E3779B1" in text and "0x85EBCA77" in text


def test_no_symbol_shared_with_the_other_eleven():
    from ngp_pl_amd import (_abi, _lib, _mesh_lib, _meshcull_lib, _meshdecimate_lib, _meshdist_lib, _meshfilter_lib, _meshquadric_lib,
                            _meshsimplify_lib, _meshsmooth_lib, _meshtex_lib, _meshtsdf_lib, _metrics_lib)
    others = (_lib, _mesh_lib, _meshfilter_lib, _meshcull_lib, _meshsimplify_lib, _meshtsdf_lib, _meshsmooth_lib, _meshtex_lib, _metrics_lib,
              _meshdist_lib, _meshquadric_lib)
    own = _exports(_meshdecimate_lib.LIB_PATH)
    assert own and not [s for s in own if not s.startswith("ngp_meshdecimate_")]
    declared = set(_abi.parse(HEADER))
    for m in others:
        theirs = _exports(m.LIB_PATH)
        assert theirs and not own & theirs and not [s for s in theirs if s.startswith("ngp_meshdecimate")]
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "ngp_meshdecimate.h":
            assert not declared & set(_abi.parse(os.path.join(ROOT, "include", h))), h


def test_ctypes_agrees_with_the_header():
    from ngp_pl_amd import _abi, _meshdecimate_lib
    protos = _abi.parse(HEADER)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _meshdecimate_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    lib = _meshdecimate_lib.lib()
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        want = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret]
        assert f.restype is want, name


def test_code_object_is_gfx950_only():
    from ngp_pl_amd import _meshdecimate_lib
    blob = open(_meshdecimate_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob


def test_build_entry_compiles_without_contraction():
    from ngp_pl_amd import build
    assert build.MESHDECIMATE_LIB == os.path.join(build.CSRC, "libngp_meshdecimate.so")
    assert "-ffp-contract=off" in build.MESHDECIMATE_CFLAGS and build.ARCH == "gfx950"
    for rel in build.MESHDECIMATE_SOURCES + build.MESHDECIMATE_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, rel)), rel


def test_argument_validation_needs_no_gpu():
    from ngp_pl_amd import _lib, _meshdecimate_lib
    lib = _meshdecimate_lib.lib()
    V, F = 100000, 180000
    ws = lib.ngp_meshdecimate_workspace_bytes(V, F)
    assert 45 * V + 24 * F <= ws < 45 * V + 24 * F + 12 * (V + F) // 2048 + 20 * 256 and ws % 256 == 0
    assert lib.ngp_meshdecimate_workspace_bytes(0, 0) >= 256
    max_f = _meshdecimate_lib.MAX_FACES
    for v, f in ((-1, 5), (5, -1), (2 ** 31, 5), (5, max_f + 1)):
        assert lib.ngp_meshdecimate_workspace_bytes(v, f) == 0
    assert lib.ngp_meshdecimate_workspace_bytes(2 ** 31 - 1, max_f) >= 45 * (2 ** 31 - 1) + 24 * max_f
    fake = C.c_void_p(4096)          # never dereferenced: every call below is rejected before a launch
    big = 2 ** 31

    def begin(faces=fake, n_v=V, n_f=F, w=fake, wb=ws):
        return ("ngp_meshdecimate_begin", faces, n_v, n_f, w, wb, None)

    def round_(vertices=fake, n_v=V, n_f=F, cell=0.5, e=-1.0, w=fake, wb=ws, totals=fake):
        return ("ngp_meshdecimate_round", vertices, n_v, n_f, cell, e, w, wb, totals, None)

    def apply(n_v=V, n_f=F, n_w=10, n_k=5, w=fake, wb=ws):
        return ("ngp_meshdecimate_apply", n_v, n_f, n_w, n_k, w, wb, None)

    def count(n_v=V, n_f=F, w=fake, wb=ws, totals=fake):
        return ("ngp_meshdecimate_count", n_v, n_f, w, wb, totals, None)

    def emit(vertices=fake, normals=None, colors=None, n_v=V, n_f=F, w=fake, wb=ws, ov=10, of=10, vo=fake, no=None, co=None, fo=fake):
        return ("ngp_meshdecimate_emit", vertices, normals, colors, n_v, n_f, w, wb, ov, of, vo, no, co, fo, None)

    nan, inf = float("nan"), float("inf")
    bad = [
        begin(faces=None), begin(w=None), begin(n_v=-1), begin(n_f=-1), begin(wb=ws - 1), begin(wb=0),
        round_(vertices=None), round_(w=None), round_(totals=None), round_(n_v=-1), round_(n_f=-1), round_(wb=ws - 1),
        round_(cell=0.0), round_(cell=-1.0), round_(cell=nan), round_(cell=inf), round_(cell=1e-50), round_(e=nan), round_(e=inf),
        round_(e=-inf),
        apply(w=None), apply(n_v=-1), apply(n_f=-1), apply(n_k=-1), apply(n_k=11), apply(n_w=V + 1, n_k=V + 1), apply(wb=ws - 1),
        count(w=None), count(totals=None), count(n_v=-1), count(n_f=-1), count(wb=ws - 1),
        emit(vertices=None), emit(w=None), emit(vo=None), emit(fo=None), emit(normals=fake), emit(no=fake), emit(colors=fake), emit(co=fake),
        emit(n_v=-1), emit(n_f=-1), emit(ov=-1), emit(of=-1), emit(ov=V + 1), emit(of=F + 1), emit(wb=ws - 1),
    ]
    for args in bad:
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshdecimate_lib.call(*args)
    for args in [begin(n_v=big), begin(n_f=max_f + 1), round_(n_v=big), round_(n_f=max_f + 1), apply(n_v=big), apply(n_f=max_f + 1),
                 count(n_v=big), count(n_f=big), emit(n_v=big), emit(n_f=max_f + 1, of=0)]:
        with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
            _meshdecimate_lib.call(*args)
    # nothing to launch
    assert _meshdecimate_lib.call(*begin(faces=None, n_v=0, n_f=0, w=None, wb=0)) == 0
    assert _meshdecimate_lib.call(*begin(faces=None, n_v=7, n_f=0, w=None, wb=0)) == 0
    assert _meshdecimate_lib.call(*apply(n_w=10, n_k=0, w=None, wb=0)) == 0
    assert _meshdecimate_lib.call(*emit(vertices=None, w=None, wb=0, ov=0, of=0, vo=None, fo=None)) == 0


def test_python_api_argument_checks():
    import torch
    from ngp_pl_amd import mesh
    v = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.decimate(mesh.Mesh(v, f), 0.5, target_faces=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.decimate(mesh.Mesh(v, f), 0.5, max_error=0.0)
    with pytest.raises(ValueError, match="target_faces, max_error or both"):
        mesh.decimate(mesh.Mesh(v, f), 0.5)
    for bad in (f.long(), f.float(), torch.zeros(2, 4, dtype=torch.int32), f.numpy()):
        with pytest.raises(ValueError):
            mesh.decimate(mesh.Mesh(v, bad), 0.5, target_faces=1)
    with pytest.raises(ValueError):
        mesh.decimate(mesh.Mesh(v.double(), f), 0.5, target_faces=1)
    for cell in (0, -1.0, float("nan"), float("inf"), 1e-50, 1e39, "x", None):
        with pytest.raises(ValueError):
            mesh.decimate(mesh.Mesh(v, f), cell, target_faces=1)
    for target in (-1, 1.5, "3", True):
        with pytest.raises(ValueError, match="target_faces"):
            mesh.decimate(mesh.Mesh(v, f), 0.5, target_faces=target)
    for e in (-1.0, float("nan"), float("inf"), 1e39, "x"):
        with pytest.raises(ValueError, match="max_error"):
            mesh.decimate(mesh.Mesh(v, f), 0.5, max_error=e)
    for opt in (-1, 2.5, dict(), dict(faces=3), dict(target_faces=-2), dict(max_error=-1.0), dict(target_faces=5, max_error=float("nan"))):
        with pytest.raises(ValueError):
            mesh.extract_mesh(None, 8, decimate=opt)


def test_cli_help_lists_the_flags(capsys):
    from ngp_pl_amd import mesh
    with pytest.raises(SystemExit) as e:
        mesh.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert re.search(r"--decimate-faces N\b", text) and re.search(r"--decimate-max-error VOXELS\b", text)
    for argv, flag in ((["--decimate-faces", "-1"], "--decimate-faces"), (["--decimate-faces", "1.5"], "--decimate-faces"),
                       (["--decimate-faces"], "--decimate-faces"), (["--decimate-max-error", "-0.5"], "--decimate-max-error"),
                       (["--decimate-max-error", "nan"], "--decimate-max-error"), (["--decimate-max-error", "inf"], "--decimate-max-error")):
        with pytest.raises(SystemExit) as e:
            mesh.main(["--ckpt", "x", "--out", "y.ply"] + argv)
        assert e.value.code == 2
        assert flag in capsys.readouterr().err


# ---- the restatement


def test_key_code_and_hash():
    c = np.array([0, 1, 2, 3, 2 ** 23, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 40 + 12345, 2 ** 56], np.int64)
    k = DR.code(c).astype(np.int64)
    assert (np.diff(k) >= 0).all() and k[0] == 0 and k[1] == 1 << 23 and k[6] == k[7] and k[7] < k[8] and k.max() < 2 ** 31
    u = np.arange(1 << 16)
    assert len(np.unique(DR.mix(u))) == len(u) and DR.mix(u).dtype == np.uint32


@pytest.mark.parametrize("n", [4, 5, 6])
def test_a_closed_fan_by_hand(n):
    v, f = fan(n)
    ov, of, _, _, st = DR.decimate(v, f, 1.0, max_error=0.0)
    # every target is valid at cost 0 on the plane: the nearest ring vertex, 1, takes the centre; its own two faces go
    assert st["totals"].tolist() == [[1, 1, n, 1], [0, 0, n - 2, 0]] and st["rounds"] == 1 and st["reached"]
    assert np.array_equal(ov, v[1:])
    assert of.tolist() == [[0, i, (i + 1) % n] for i in range(1, n - 1)]      # (1, 1 + i, 2 + i) re-indexed
    key, target, won, totals = DR.evaluate(v, DR.begin(f, len(v)), 1.0, 0.0)
    assert target.tolist() == [1] + [-1] * n and won.tolist() == [True] + [False] * n and key[0] == DR.mix(0)
    # off the plane by more than the bound: nothing; within a generous bound: the same collapse, at a cost
    v[0, 2] = 0.25
    assert DR.decimate(v, f, 1.0, max_error=0.01)[4]["totals"].tolist() == [[0, 0, n, 0]]
    lifted = DR.decimate(v, f, 1.0, max_error=0.5)
    assert np.array_equal(lifted[1], of) and (DR.evaluate(v, DR.begin(f, len(v)), 1.0, 0.5)[0][0] >> np.uint64(32)) > 0
    # a budget instead of a bound
    assert np.array_equal(DR.decimate(v, f, 1.0, target_faces=n - 1)[1], of)
    same = DR.decimate(v, f, 1.0, target_faces=n)
    assert same[0] is v and np.array_equal(same[1], f)


def test_boundary_bow_tie_and_tetrahedron_do_not_collapse():
    v, f = fan(6, open_at=2)
    ov, of, _, _, st = DR.decimate(v, f, 1.0, target_faces=2)
    assert np.array_equal(ov, v) and np.array_equal(of, f) and st["totals"].tolist() == [[0, 0, 5, 0]] and not st["reached"]
    # two closed fans that share their centre: a bow-tie
    v2, f2 = fan(5, z=1.0)
    vb = np.concatenate([v, v2[1:]])
    fb = np.concatenate([fan(6)[1], np.where(f2 == 0, 0, f2 + 6)]).astype(np.int32)
    assert not DR.removable(vb, *DR.corners(DR.begin(fb, len(vb)), len(vb))[1:])[0]
    assert DR.decimate(vb, fb, 1.0, target_faces=2)[4]["totals"].tolist() == [[0, 0, 11, 0]]
    # a tetrahedron: every vertex is removable, every collapse would double the opposite face
    v, f = tetrahedron()
    assert DR.removable(v, *DR.corners(DR.begin(f, 4), 4)[1:]).all()
    ov, of, _, _, st = DR.decimate(v, f, 1.0, target_faces=2)
    assert np.array_equal(of, f) and st["totals"].tolist() == [[0, 0, 4, 0]] and not st["reached"]


@pytest.mark.parametrize("n", [12, 24])
def test_a_box_collapses_to_its_corners(n):
    v, f = G.box(n)
    ov, of, _, _, st = box_decimated(n)
    print("box(%d): %d rounds" % (n, st["rounds"]))
    assert ov.shape == (8, 3) and of.shape == (12, 3) and st["reached"] and st["totals"][-1].tolist() == [0, 0, 12, 0]
    idx = input_index(v, ov)
    assert (np.diff(idx) > 0).all()                                            # input vertices, in input order
    lo, hi = G.BOX_LO.astype(np.float32), G.BOX_HI.astype(np.float32)
    assert ((ov == lo) | (ov == hi)).all() and len(np.unique(ov, axis=0)) == 8
    p = ov[of]
    on_side = [(p[:, :, k] == s[k]).all(1) for k in range(3) for s in (lo, hi)]
    assert np.stack(on_side).sum(0).tolist() == [1] * 12                       # every face on exactly one side
    assert R.is_closed_oriented(of) and R.euler(ov, of) == 2
    assert abs(R.signed_volume(ov, of) - R.signed_volume(v, f)) < 1e-6 and G.box_distance(p.mean(1)).max() < 5e-8


@pytest.mark.parametrize("K", [2, 3])
def test_the_sphere_to_the_face_count_of_the_clustering(K):
    v, f = sphere()
    cv, cf = cluster_faces(K)
    ov, of, _, _, st = sphere_decimated(K)
    assert len(of) == len(cf) == {2: 2964, 3: 1410}[K] and st["reached"] and st["faces"] == len(of)
    assert R.is_closed_oriented(of) and R.euler(ov, of) == 2 and R.signed_volume(ov, of) > 0
    assert (np.diff(input_index(v, ov)) > 0).all() and of.max() == len(ov) - 1
    (dm, dx), (cm, cx) = surface_error(ov, of), surface_error(cv, cf)
    print("sphere K=%d: %d rounds; decimated mean %.3e max %.3e, clustered mean %.3e max %.3e, ratio %.3f" % (
        K, st["rounds"], dm, dx, cm, cx, dm / cm))
    assert dm < cm
    t = st["totals"]
    assert (t[:-1, 2] - 2 * t[:-1, 3] == t[1:, 2]).all()                       # two faces per applied collapse


def test_an_open_cap_keeps_its_boundary():
    v, f = cap()
    edges = boundary_edges(f)
    rim = sorted({i for e in edges for i in e})
    assert len(rim) > 50 and len(edges) == len(rim)
    ov, of, _, _, st = DR.decimate(v, f, SPHERE_CELL, target_faces=len(f) // 3)
    assert st["reached"] and len(f) // 3 - 1 <= len(of) <= len(f) // 3
    idx = input_index(v, ov)
    assert set(rim) <= set(idx.tolist())
    assert {tuple(sorted(e)) for e in idx[np.array(sorted(boundary_edges(of)))].tolist()} == edges


def test_a_permutation_of_the_faces_changes_nothing():
    v, f = sphere()
    f = f[:4000]                                                               # open, with a long boundary
    g = np.random.RandomState(4)
    a = DR.decimate(v, f, SPHERE_CELL, target_faces=1500)
    b = DR.decimate(v, f[g.permutation(len(f))], SPHERE_CELL, target_faces=1500)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[4]["totals"], b[4]["totals"]) and len(a[1]) <= 1500
    canon = lambda t: np.unique(np.stack([np.roll(r, -int(r.argmin())) for r in t]), axis=0)
    assert np.array_equal(canon(a[1]), canon(b[1]))
