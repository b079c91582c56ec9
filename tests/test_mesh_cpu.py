"""CPU: the marching-cubes table generator and its committed header, the C ABI of libngp_mesh.so (header, exports, ctypes, code
object, host-side argument checks) and the PLY writer.  libngp_hip.so's own symbol set is pinned by tests/test_capi_cpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ngp_pl_amd import mc_tables as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_HEADER = os.path.join(ROOT, "include", "ngp_mesh.h")


def test_generator_reproduces_the_committed_header():
    assert open(T.HEADER).read() == T.render()


def test_triangles_use_exactly_the_sign_change_edges():
    _, tris, _ = T.tables()
    for c in range(256):
        assert sorted({e for t in tris[c] for e in t}) == T.sign_change_edges(c), c
        assert all(len(set(t)) == 3 for t in tris[c]), c
    assert not tris[0] and not tris[255]


def test_triangle_boundary_is_the_face_rule():
    """The boundary of a case's triangles is exactly the prescribed face segments, each once and in its direction; every other
    triangle edge (a fan diagonal) is used twice, once in each direction, and joins two edges that share no cube face."""
    _, tris, _ = T.tables()
    for c in range(256):
        use = {}
        for t in tris[c]:
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                use[(a, b)] = use.get((a, b), 0) + 1
        boundary = sorted(k for k in use if (k[1], k[0]) not in use)
        assert boundary == sorted(T.case_segments(c)), c
        assert all(v == 1 for v in use.values()), c
        for a, b in use:
            if (b, a) in use:
                assert not T._share_face(a, b), (c, a, b)


def test_face_rule_keeps_diagonal_inside_corners_apart():
    # face z=0 with inside corners 0 and 3 (a diagonal): two segments, each cutting off one corner
    face = [f for f in T.FACES if f[0] == 2 and f[1] == 0][0]
    segs = T.face_segments(0b1001, face)
    assert sorted(sorted(s) for s in segs) == [[0, 4], [1, 5]]


def test_single_corner_triangle_faces_outward():
    # corner 0 inside: the triangle over edges x, y, z from corner 0 winds x -> y -> z, normal (1, 1, 1) pointing away from it
    assert T.case_triangles(1) == [(0, 4, 8)]


def test_headers_compile_as_c99():
    for src in ('#include "ngp_mesh.h"\nint main(void) { return 0; }\n',
                '#include "ngp_hip.h"\n#include "ngp_mesh.h"\nint main(void) { return 0; }\n',
                '#include "../ngp_pl_amd/csrc/mesh/mc_tables.h"\nint main(void) { return NGP_MC_TRIS[1][0] + NGP_MC_TRI_COUNT[1] + '
                'NGP_MC_EDGE_MASK[1] + NGP_MC_EDGE_CORNERS[0][0]; }\n'):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout


def test_mesh_library_exports_exactly_its_header():
    from ngp_pl_amd import _abi, _mesh_lib
    protos = _abi.parse(MESH_HEADER)
    assert len(protos) == 6
    out = subprocess.run(["nm", "-D", "--defined-only", _mesh_lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(re.findall(r" T (\w+)", out))
    assert exported == set(protos)
    assert set(_mesh_lib.exported_symbols()) == set(protos)
    assert not set(protos) & set(_abi.parse_all()), "a mesh entry point in libngp_hip.so's headers"
    lib = _mesh_lib.lib()
    assert lib.ngp_mesh_abi_version() == 1 == _mesh_lib.ABI_VERSION and lib.ngp_mesh_build_arch() == b"gfx950"


def test_main_library_exports_no_mesh_symbol():
    from ngp_pl_amd import _lib
    _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert not re.findall(r" T (ngp_mesh\w*)", out)


def test_ctypes_agrees_with_the_mesh_header():
    from ngp_pl_amd import _abi, _mesh_lib
    protos = _abi.parse(MESH_HEADER)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _mesh_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    lib = _mesh_lib.lib()
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        want = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret]
        assert f.restype is want, name


def test_mesh_code_object_is_gfx950_only():
    from ngp_pl_amd import _mesh_lib
    blob = open(_mesh_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob


def test_argument_validation_needs_no_gpu():
    from ngp_pl_amd import _lib, _mesh_lib
    lib = _mesh_lib.lib()
    ws = lib.ngp_mesh_workspace_bytes(64, 64, 64)
    assert 5 * 64 ** 3 <= ws < 5 * 64 ** 3 + 4096
    assert lib.ngp_mesh_workspace_bytes(1, 64, 64) == 0 and lib.ngp_mesh_workspace_bytes(64, 65536, 64) == 0
    fake = C.c_void_p(4096)          # never dereferenced: every call below is rejected before a launch
    b6 = _mesh_lib.bounds6((0, 0, 0), (1, 1, 1))
    bad = [
        ("ngp_mesh_count", None, 64, 64, 64, 20.0, fake, ws, fake, None),               # null volume
        ("ngp_mesh_count", fake, 64, 64, 64, 20.0, None, ws, fake, None),               # null workspace
        ("ngp_mesh_count", fake, 64, 64, 64, 20.0, fake, ws, None, None),               # null totals
        ("ngp_mesh_count", fake, 1, 64, 64, 20.0, fake, ws, fake, None),                # axis below 2
        ("ngp_mesh_count", fake, 64, 64, 70000, 20.0, fake, ws, fake, None),            # axis above 65535
        ("ngp_mesh_count", fake, 64, 64, 64, 20.0, fake, ws - 1, fake, None),           # workspace too small
        ("ngp_mesh_emit", fake, 64, 64, 64, 20.0, None, fake, ws, 1, 1, fake, fake, fake, None),    # null bounds
        ("ngp_mesh_emit", fake, 64, 64, 64, 20.0, b6, fake, ws, 1, 1, None, fake, fake, None),      # null vertices
        ("ngp_mesh_emit", fake, 64, 64, 64, 20.0, b6, fake, ws, 1, 1, fake, fake, None, None),      # null faces
        ("ngp_mesh_emit", fake, 64, 64, 64, 20.0, b6, fake, ws, -1, 1, fake, fake, fake, None),     # negative count
        ("ngp_mesh_emit", fake, 64, 64, 64, 20.0, _mesh_lib.bounds6((0, 0, 0), (1, 0, 1)), fake, ws, 1, 1, fake, fake, fake, None),
        ("ngp_mesh_lattice_points", 64, 64, 64, b6, 0, 64 ** 3 + 1, fake, None),       # range past the lattice
        ("ngp_mesh_lattice_points", 64, 64, 64, b6, -1, 1, fake, None),
        ("ngp_mesh_lattice_points", 64, 64, 64, b6, 0, 1, None, None),
    ]
    for args in bad:
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _mesh_lib.call(*args)
    with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
        _mesh_lib.call("ngp_mesh_emit", fake, 64, 64, 64, 20.0, b6, fake, ws, 2 ** 31, 1, fake, fake, fake, None)
    assert _mesh_lib.call("ngp_mesh_emit", fake, 64, 64, 64, 20.0, b6, fake, ws, 0, 0, None, None, None, None) == 0   # empty mesh
    assert _mesh_lib.call("ngp_mesh_lattice_points", 64, 64, 64, b6, 5, 0, None, None) == 0


def test_python_api_rejects_cpu_tensors_and_bad_resolution():
    import torch
    from ngp_pl_amd import mesh
    with pytest.raises(RuntimeError, match="CUDA"):
        mesh.marching_cubes(torch.zeros(4, 4, 4), 0.5)
    with pytest.raises(ValueError):
        mesh._resolution(1)
    with pytest.raises(ValueError):
        mesh._resolution((4, 4))


def read_ply(path):
    """Minimal reader of the binary little-endian PLY save_ply writes."""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    head = blob[:end].decode("ascii").splitlines()
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    elems, cur = [], None
    for line in head[2:-1]:
        w = line.split()
        if w[0] == "element":
            cur = [w[1], int(w[2]), []]
            elems.append(cur)
        elif w[0] == "property":
            cur[2].append(w[1:])
    off, out = end, {}
    for name, n, props in elems:
        if name == "vertex":
            dt = np.dtype([(p[1], {"float": "<f4", "uchar": "u1"}[p[0]]) for p in props])
            out["vertex"] = np.frombuffer(blob, dt, n, off)
        else:
            assert props == [["list", "uchar", "int", "vertex_indices"]]
            dt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
            out["face"] = np.frombuffer(blob, dt, n, off)
        off += dt.itemsize * n
    assert off == len(blob)
    return out


@pytest.mark.parametrize("with_colors", [False, True])
def test_ply_round_trip(tmp_path, with_colors):
    from ngp_pl_amd import mesh
    g = np.random.RandomState(0)
    v = g.randn(50, 3).astype(np.float32)
    n = g.randn(50, 3).astype(np.float32)
    f = g.randint(0, 50, (70, 3)).astype(np.int32)
    c = g.rand(50, 3).astype(np.float32) if with_colors else None
    p = tmp_path / "m.ply"
    mesh.save_ply(str(p), mesh.Mesh(v, f, n, c))
    r = read_ply(str(p))
    vv = r["vertex"]
    assert np.array_equal(np.stack([vv["x"], vv["y"], vv["z"]], 1), v)
    assert np.array_equal(np.stack([vv["nx"], vv["ny"], vv["nz"]], 1), n)
    assert (r["face"]["n"] == 3).all() and np.array_equal(r["face"]["v"], f)
    if with_colors:
        assert np.array_equal(np.stack([vv["red"], vv["green"], vv["blue"]], 1), np.round(c * 255).astype(np.uint8))
    else:
        assert "red" not in vv.dtype.names


def test_numpy_restatement_is_closed_on_every_case():
    """The CPU restatement the GPU tests compare against: on bordered noise every cube index occurs and the mesh is closed and
    consistently oriented."""
    from tests import mc_reference as R
    g = np.random.RandomState(1)
    v = g.rand(40, 40, 40).astype(np.float32)
    v[[0, -1]] = 0
    v[:, [0, -1]] = 0
    v[:, :, [0, -1]] = 0
    verts, faces, _, cube = R.marching_cubes(v, 0.5, (0, 0, 0), (1, 1, 1))
    assert len(np.unique(cube)) == 256
    assert R.is_closed_oriented(faces)
