"""CPU: the C ABI of libngp_meshnormal.so (header, exports, ctypes, code object, build entry, host-side refusals), the Python
surface's argument checks, extract_mesh's option parsing, the OBJ writer and the CLI's refusals, and the numpy restatement the GPU
tests compare against (tests/mesh_normal_reference.py): the seven regions of the unit right triangle, the thin wall worked by
hand, the f32 rule against the float64 definition, and two quality conditions (a rippled sheet, a sphere)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_distance_reference as DR
from tests import mesh_normal_reference as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN = os.path.join(ROOT, "ngp_pl_amd", "csrc", "meshnormal")           # the header lies beside the sources
HEADER = os.path.join(OWN, "ngp_meshnormal.h")
ENTRY_POINTS = ("abi_version", "build_arch", "transfer", "shade")
F = np.float32


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


# ---- 1. the C ABI


def test_header_compiles_as_c99_alone_and_after_meshdist():
    for src in ('#include "ngp_meshnormal.h"\nint main(void) { return NGP_EINVAL + NGP_ERANGE + NGP_MESHNORMAL_MAX_SHELLS; }\n',
                '#include "ngp_meshdist.h"\n#include "ngp_meshnormal.h"\nint main(void) { return NGP_MESHNORMAL_SLACK_ULPS - NGP_MESHDIST_SLACK_ULPS; }\n',
                '#include "ngp_meshnormal.h"\n#include "ngp_meshdist.h"\nint main(void) { return NGP_MESHNORMAL_SCAN_BLOCK - NGP_MESHDIST_SCAN_BLOCK; }\n'):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-I", OWN, "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}         # it restates what it uses
    assert "#ifndef NGP_EINVAL" in text and "#ifndef NGP_ERANGE" in text and "THE RULE" in text and "THE CAP" in text
    from ngp_pl_amd import _meshdist_lib, _meshnormal_lib as L
    for name, value in (("MAX_SHELLS", 8), ("MAX_AXIS", _meshdist_lib.MAX_AXIS), ("MAX_CELLS", _meshdist_lib.MAX_CELLS),
                        ("SLACK_ULPS", _meshdist_lib.SLACK_ULPS), ("MIN_CELL_SLACKS", _meshdist_lib.MIN_CELL_SLACKS),
                        ("SCAN_BLOCK", _meshdist_lib.SCAN_BLOCK)):
        assert getattr(L, name) == value and re.search(r"#define NGP_MESHNORMAL_%s %d\s" % (name, value), text), name
    assert NR.MAX_SHELLS == L.MAX_SHELLS


def test_library_exports_exactly_its_header_and_the_abi_version():
    from ngp_pl_amd import _abi, _meshnormal_lib as L
    protos = _abi.parse(HEADER)
    assert set(protos) == {"ngp_meshnormal_" + n for n in ENTRY_POINTS}
    assert _exports(L.LIB_PATH) == set(protos) == set(L.exported_symbols())
    lib = L.lib()
    assert lib.ngp_meshnormal_abi_version() == 1 == L.ABI_VERSION and lib.ngp_meshnormal_build_arch() == b"gfx950"
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in L._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    assert [p.name for p in protos["ngp_meshnormal_transfer"].params] == [
        "points", "query_normals", "valid", "n", "vertices", "faces", "vertex_normals", "n_vertices", "n_faces", "origin", "cell", "nx", "ny",
        "nz", "workspace", "workspace_bytes", "entries", "n_entries", "max_dist", "oriented", "normals_out", "d2", "face", "bary", "debug", "stream"]
    assert [p.name for p in protos["ngp_meshnormal_shade"].params] == ["albedo", "samples", "ids", "lights", "n_cams", "H", "W", "ambient", "out", "stream"]


def test_no_symbol_is_shared_with_the_other_libraries():
    from ngp_pl_amd import (_lib, _mesh_lib, _meshatlas_lib, _meshcull_lib, _meshdecimate_lib, _meshdist_lib, _meshfilter_lib, _meshnormal_lib,
                            _meshphoto_lib, _meshquadric_lib, _meshsimplify_lib, _meshsmooth_lib, _meshtex_lib, _meshtsdf_lib, _metrics_lib)
    others = (_lib, _mesh_lib, _meshfilter_lib, _meshcull_lib, _meshsimplify_lib, _meshtsdf_lib, _meshsmooth_lib, _meshtex_lib, _metrics_lib,
              _meshdist_lib, _meshquadric_lib, _meshdecimate_lib, _meshatlas_lib, _meshphoto_lib)
    assert len({m.LIB_PATH for m in others + (_meshnormal_lib,)}) == 15
    own = _exports(_meshnormal_lib.LIB_PATH)
    assert own and all(s.startswith("ngp_meshnormal_") for s in own)
    for m in others:
        theirs = _exports(m.LIB_PATH)
        assert theirs and not own & theirs and not [s for s in theirs if s.startswith("ngp_meshnormal")], m.LIB_PATH


def test_code_object_and_build_entry():
    from ngp_pl_amd import _meshnormal_lib as L, build
    blob = open(L.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob
    for kernel in (b"transfer", b"shade"):
        assert kernel in blob
    assert build.MESHNORMAL_LIB == L.LIB_PATH and build.MESHNORMAL_CFLAGS == ["-ffp-contract=off"] and build.ARCH == "gfx950"
    assert build.MESHNORMAL_SOURCES == [os.path.join("meshnormal", "meshnormal.hip")]
    for rel in build.MESHNORMAL_SOURCES + build.MESHNORMAL_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, rel)), rel
    source = open(os.path.join(build.CSRC, build.MESHNORMAL_SOURCES[0])).read()
    # no other library's ABI header or source is compiled in: only the walk's device code, shared with libngp_meshdist.so, and
    # the host helpers every mesh library shares
    assert set(re.findall(r'#include\s*"([^"]+)"', source)) == {"ngp_meshnormal.h", "../mesh_nearest.h", "../mesh_host.h"}
    assert "constexpr int THREADS = 256;" in source


# ---- 2. host refusals through the library, no GPU


def _ws_bytes(dims):
    cells = dims[0] * dims[1] * dims[2]
    return 8 * ((cells + 2047) // 2048) + 4 * (cells + 1) + 4 * cells


def test_host_refusals_need_no_gpu():
    """A refused call never launches; an accepted one is made with n == 0, which launches nothing (every other argument is still
    checked), so both sides of every limit are exercised without a GPU."""
    from ngp_pl_amd import _lib, _meshdist_lib, _meshnormal_lib as L
    fake = C.c_void_p(4096)          # never dereferenced
    inf, nan = float("inf"), float("nan")
    up = lambda x: float(np.nextafter(F(x), F(np.inf)))

    def transfer(points=fake, qn=fake, valid=fake, n=100, v=fake, f=fake, vn=fake, n_v=10, n_f=5, origin=(0, 0, 0), cell=0.5, dims=(4, 3, 2),
                 ws=fake, ws_bytes=None, entries=fake, n_entries=7, max_dist=1.0, oriented=1, out=fake, d2=fake, face=fake, bary=fake, debug=fake):
        ws_bytes = _ws_bytes(dims) if ws_bytes is None else ws_bytes
        return ("ngp_meshnormal_transfer", points, qn, valid, n, v, f, vn, n_v, n_f, None if origin is None else L.floats(origin), cell,
                dims[0], dims[1], dims[2], ws, ws_bytes, entries, n_entries, max_dist, oriented, out, d2, face, bary, debug, None)

    cell = float(F(0.5))
    for kw in (dict(), dict(max_dist=0.0), dict(max_dist=8 * cell), dict(oriented=0, max_dist=8 * cell), dict(bary=None, debug=None),
               dict(dims=(1, 1, 1)), dict(dims=(1024, 1024, 1024), cell=1.0), dict(n_entries=0, entries=None), dict(n_f=0, f=None),
               dict(n_v=0, v=None, vn=None), dict(points=None, qn=None, valid=None, out=None, d2=None, face=None)):
        assert L.call(*transfer(n=0, **kw)) == 0, kw
    # the workspace the library asks for is the one libngp_meshdist.so lays out
    for dims in ((4, 3, 2), (1, 1, 1), (64, 64, 64), (1024, 3, 700)):
        assert _ws_bytes(dims) == _meshdist_lib.lib().ngp_meshdist_grid_workspace_bytes(*dims)
    refused = [dict(max_dist=inf), dict(max_dist=-inf), dict(max_dist=nan), dict(max_dist=-1.0), dict(max_dist=up(8 * cell)),        # THE CAP
               dict(max_dist=inf, oriented=0), dict(max_dist=up(8 * cell), oriented=0), dict(max_dist=3.4e38),
               dict(dims=(0, 3, 2)), dict(dims=(4, 1025, 2)), dict(dims=(4, 3, -1)), dict(dims=(1024, 1024, 1024), cell=1.0, ws_bytes=2 ** 33),  # 2^30 cells are the limit ...
               dict(cell=0.0), dict(cell=-0.5), dict(cell=inf), dict(cell=nan), dict(origin=(0, nan, 0)), dict(origin=(inf, 0, 0)), dict(origin=None),
               dict(origin=(1e6, 0, 0), cell=0.05, max_dist=0.1),                                     # the cell below 2^-14 of the grid's magnitude
               dict(ws_bytes=_ws_bytes((4, 3, 2)) - 1), dict(ws=C.c_void_p(4100)), dict(ws=None),
               dict(n_v=-1), dict(n_f=-1), dict(n_entries=-1)]
    refused[11] = dict(dims=(1024, 1024, 1025), cell=1.0, ws_bytes=2 ** 34)                           # ... and more than 2^30 are refused
    for kw in refused:
        for n in (0, 100):           # refused whether or not there is anything to do (n = 100 is reached only once n = 0 was refused)
            with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
                L.call(*transfer(**dict(kw, n=n)))
    with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
        L.call(*transfer(n=-1))
    for name in ("points", "qn", "valid", "v", "f", "vn", "entries", "out", "d2", "face"):          # null pointers with positive sizes
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            L.call(*transfer(**{name: None}))
    for kw in (dict(n=2 ** 31), dict(n_v=2 ** 31), dict(n_f=2 ** 31), dict(n_entries=2 ** 31)):
        with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
            L.call(*transfer(**kw))

    def shade(albedo=fake, samples=fake, ids=fake, lights=fake, n_cams=2, H=12, W=16, ambient=0.25, out=fake):
        return ("ngp_meshnormal_shade", albedo, samples, ids, lights, n_cams, H, W, ambient, out, None)

    for kw in (dict(), dict(ambient=0.0), dict(ambient=1.0), dict(W=1, H=1), dict(W=16384, H=16384), dict(albedo=None, samples=None, ids=None, lights=None, out=None)):
        assert L.call(*shade(n_cams=0, **kw)) == 0, kw
    for kw in (dict(ambient=-0.1), dict(ambient=up(1.0)), dict(ambient=nan), dict(W=0), dict(H=0), dict(W=16385), dict(H=-3), dict(n_cams=-1)):
        for n_cams in (0, 2):
            with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
                L.call(*shade(**dict(dict(n_cams=n_cams), **kw)))
    for name in ("albedo", "samples", "ids", "lights", "out"):
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            L.call(*shade(**{name: None}))
    with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
        L.call(*shade(n_cams=9, W=16384, H=16384))


# ---- 3. the Python surface without a GPU


def _cpu_mesh():
    import torch
    from ngp_pl_amd import mesh
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=torch.float32)
    f = torch.tensor([[0, 1, 2], [1, 3, 2]], dtype=torch.int32)
    n = torch.tensor([[0, 0, 1.0]] * 4)
    return mesh, mesh.Mesh(v, f, n)


def test_python_argument_checks():
    import torch
    mesh, m = _cpu_mesh()
    pts, nrm = torch.zeros(5, 3), torch.ones(5, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.transfer_normals(pts, nrm, m, 0.5)
    with pytest.raises(ValueError, match="texture"):
        mesh.bake_normal_map(m, m, 0.5)
    for bad in (float("inf"), float("nan"), -1.0, None, "1", True, 1e39):
        with pytest.raises(ValueError, match="max_dist"):
            mesh._max_dist(bad)
    assert mesh._max_dist(0.1) == float(F(0.1)) and mesh._max_dist(0) == 0.0
    for chunk in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="chunk"):
            mesh.bake_normal_map(m, m, 0.5, chunk=chunk)
    for light in ((0, 0, 0), (1, 2), "abc", (float("nan"), 0, 1), (float("inf"), 0, 0), 3.0):
        with pytest.raises(ValueError, match="light"):
            mesh._light(light)
    assert np.array_equal(mesh._light((0, 3, 4)), F([0, 0.6, 0.8])) and np.array_equal(mesh._light((0.3, 0.5, 0.8)), NR.light_f32((0.3, 0.5, 0.8)))
    for ambient in (-0.1, 1.5, float("nan"), None, True):
        with pytest.raises(ValueError, match="ambient"):
            mesh._ambient(ambient)
    # the field lists the other tests pin are as they were; the new class adds one field
    import dataclasses
    assert [x.name for x in dataclasses.fields(mesh.Mesh)] == ["vertices", "faces", "normals", "colors", "texture"]
    assert [x.name for x in dataclasses.fields(mesh.NormalMappedMesh)] == ["vertices", "faces", "normals", "colors", "texture", "normal_map"]
    assert [x.name for x in dataclasses.fields(mesh.NormalMap)] == ["image", "width", "height", "max_dist", "oriented", "hits", "valid"]
    assert issubclass(mesh.NormalMappedMesh, mesh.Mesh)


def test_extract_mesh_texture_options_with_a_normal_map():
    from ngp_pl_amd import mesh
    default = dict(max_dist=None, oriented=True)
    # without the option nothing changes
    assert mesh._texture_options(None) is None and mesh._texture_options(4) == 4 and mesh._texture_options(dict(texels=4)) == 4
    assert mesh._texture_options(dict(texels=4, normal_map=None)) == 4 and mesh._texture_options(dict(texels=4, normal_map=False)) == 4
    assert mesh._texture_options(dict(texel_size=2.0)) == dict(min_texels=1, max_texels=256, texel_size=2.0)
    assert mesh._texture_options(dict(texels=4, normal_map=True)) == dict(texels=4, normal_map=default)
    assert mesh._texture_options(dict(normal_map=True)) == dict(texels=8, normal_map=default)
    assert mesh._texture_options(dict(texel_size=2.0, normal_map=dict(max_dist=3, oriented=False))) == dict(
        min_texels=1, max_texels=256, texel_size=2.0, normal_map=dict(max_dist=3.0, oriented=False))
    assert mesh._texture_options(dict(max_side=512, normal_map=dict()))["normal_map"] == default
    for bad in (1, "yes", dict(max_dist=0), dict(max_dist=-1), dict(max_dist=float("inf")), dict(max_dist="4"), dict(oriented=1), dict(reach=4)):
        with pytest.raises(ValueError, match="normal_map"):
            mesh._texture_options(dict(texels=4, normal_map=bad))
    with pytest.raises(ValueError, match="simplify_voxels or decimate"):                      # refused when neither simplification runs
        mesh.extract_mesh(None, 8, texture=dict(texels=2, normal_map=True))
    with pytest.raises(ValueError, match="simplify_voxels or decimate"):
        mesh.extract_mesh(None, 8, texture=dict(texels=2, normal_map=True), smooth=3, keep_largest=1)


def test_obj_writer_round_trip_with_a_normal_map(tmp_path):
    import torch
    from tests import mesh_texture_reference as TR
    mesh, m = _cpu_mesh()
    _, w, h = TR.atlas_size(2, 2)
    g = np.random.RandomState(0)
    tex = mesh.Texture(2, w, h, 1, torch.from_numpy(TR.face_uvs(2, 2)), torch.from_numpy(g.randint(0, 256, (h, w, 3)).astype(np.uint8)))
    nm = mesh.NormalMap(torch.from_numpy(g.randint(0, 256, (h, w, 3)).astype(np.uint8)), w, h, 0.5, True, torch.tensor(3), torch.tensor(4))
    mm = mesh.NormalMappedMesh(m.vertices, m.faces, m.normals, None, tex, nm)
    plain, both = str(tmp_path / "plain.obj"), str(tmp_path / "both.obj")
    mesh.save_obj(plain, mm)                                    # the field alone changes nothing: the map is written when it is passed
    mesh.save_obj(both, mm, normal_map=mm.normal_map)
    assert sorted(os.listdir(tmp_path)) == ["both.mtl", "both.obj", "both.png", "both_normal.png", "plain.mtl", "plain.obj", "plain.png"]
    assert open(plain).read().replace("plain", "both") == open(both).read()
    assert open(str(tmp_path / "plain.png"), "rb").read() == open(str(tmp_path / "both.png"), "rb").read() == mesh._png(tex.image.numpy())
    assert open(str(tmp_path / "both_normal.png"), "rb").read() == mesh._png(nm.image.numpy())
    mtl_plain, mtl = open(str(tmp_path / "plain.mtl")).read(), open(str(tmp_path / "both.mtl")).read()
    assert mtl_plain == "newmtl plain\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd plain.png\n"       # as before this option existed
    assert mtl.startswith(mtl_plain.replace("plain", "both")) and mtl.endswith("norm both_normal.png\n")
    extra = mtl[len(mtl_plain.replace("plain", "both")):].splitlines()
    assert len(extra) == 2 and extra[0].startswith("#") and "object-space" in extra[0] and "bump" not in mtl.lower()
    with pytest.raises(ValueError, match="normal map"):
        mesh.save_obj(both, mm, normal_map=mesh.NormalMap(nm.image[:-1], w, h - 1, 0.5, True, None, None))


def test_cli_lists_the_options_and_refuses_bad_combinations(capsys):
    from ngp_pl_amd import mesh
    with pytest.raises(SystemExit) as e:
        mesh.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--texture-normal-map", "--texture-normal-max-dist VOXELS", "--texture-normal-two-sided"):
        assert flag in out
    ok = ["--out", "y.obj", "--texture-texels", "2", "--simplify-voxels", "2"]
    for bad in (["--out", "y.obj", "--texture-normal-map", "--simplify-voxels", "2"],                     # no atlas option
                ["--out", "y.ply", "--texture-normal-map", "--simplify-voxels", "2"],                     # a PLY carries no texture
                ["--out", "y.obj", "--texture-texels", "2", "--texture-normal-map"],                      # no simplification
                ["--out", "y.obj", "--texture-texels", "2", "--texture-normal-map", "--smooth-iterations", "3"],
                ok + ["--texture-normal-max-dist", "4"], ok + ["--texture-normal-two-sided"],             # the sub-options need the flag
                ok + ["--texture-normal-map", "--texture-normal-max-dist", "0"], ok + ["--texture-normal-map", "--texture-normal-max-dist", "nan"],
                ok + ["--texture-normal-map", "--texture-normal-max-dist", "-2"]):
        with pytest.raises(SystemExit) as e:
            mesh.main(["--ckpt", "x"] + bad)
        assert e.value.code == 2, bad
        assert "--texture-normal-" in capsys.readouterr().err


# ---- 4. the rule on hand-worked cases


def test_the_seven_regions_of_the_unit_right_triangle():
    a, b, c = F([[0, 0, 0]]), F([[1, 0, 0]]), F([[0, 1, 0]])
    cases = [((-1, -1, 0.5), 0, (0, 0)), ((2, -0.5, 0.5), 1, (1, 0)), ((-0.5, 2, 0.5), 3, (0, 1)),      # the vertices a, b, c
             ((0.25, -1, 0.5), 2, (0.25, 0)), ((-1, 0.75, 0.5), 4, (0, 0.75)),                          # the edges ab, ac
             ((1, 1, 0.5), 5, (0.5, 0.5)), ((1.25, 0.75, 0.5), 5, (0.75, 0.25)),                        # the edge bc: (1 - w, w)
             ((0.25, 0.5, 0.5), 6, (0.25, 0.5)), ((0.125, 0.125, -2), 6, (0.125, 0.125))]               # the interior
    for p, case, (v, w) in cases:
        q, d2, got, bv, bw = NR.pair_f32(F([p]), a, b, c)
        assert got[0] == case and (float(bv[0]), float(bw[0])) == (v, w), (p, got, bv, bw)
        assert q[0].tolist() == [v, w, 0.0]                                                             # q = a + v ab + w ac on this triangle
        assert float(d2[0]) == float((F(p[0]) - F(v)) ** 2 + (F(p[1]) - F(w)) ** 2 + F(p[2]) ** 2)
        _, dd, cc = DR.closest_f32(F([p]), a, b, c)                                                     # and the restatement meshdist's tests use agrees
        assert cc[0, 0] == case and dd[0, 0] == d2[0]
    assert sorted({c[1] for c in cases}) == list(range(7))
    # the normal: u Na + v Nb + w Nc normalised, in the interior and at a corner
    vn = F([[1, 0, 0], [0, 1, 0], [0, 0, 1]])
    n, d2, face, bary = NR.transfer_f32(F([[0.25, 0.5, 0.5], [2, -0.5, 0.5]]), F([[0, 0, 1]] * 2), None, np.concatenate([a, b, c]), [[0, 1, 2]], vn, 4.0)
    assert face.tolist() == [0, 0] and bary.tolist() == [[0.25, 0.5], [1, 0]] and n[1].tolist() == [0, 1, 0]
    L = np.sqrt(F(0.25) * F(0.25) + F(0.25) * F(0.25) + F(0.5) * F(0.5))
    assert n[0].tolist() == [float(F(0.25) / L), float(F(0.25) / L), float(F(0.5) / L)]


def test_the_thin_wall_by_hand():
    v, f, vn = NR.thin_wall()
    p, m = F([[0.3, 0.4, 0.006]]), F([[0, 0, -1]])
    lower, upper = float(F(0.006)) ** 2, None
    e = F(0.006) - F(0.01)
    upper = e * e
    n, d2, face, bary = NR.transfer_f32(p, m, None, v, f, vn, 1.0, oriented=False)                       # the z = 0.01 sheet is nearer: 0.004
    assert face[0] in (2, 3) and d2[0] == upper and abs(np.sqrt(float(d2[0])) - 0.004) < 1e-9 and n[0].tolist() == [0, 0, 1]
    n, d2, face, bary = NR.transfer_f32(p, m, None, v, f, vn, 1.0, oriented=True)                        # the z = 0 sheet faces the way m does: 0.006
    assert face[0] in (0, 1) and d2[0] == F(0.006) * F(0.006) and n[0].tolist() == [0, 0, -1]
    assert abs(np.sqrt(float(d2[0])) - 0.006) < 1e-9 and lower > float(upper)
    n, d2, face, bary = NR.transfer_f32(p, m, None, v, f, vn, 0.005, oriented=True)                      # out of reach: a miss, the fallback is m
    assert face[0] == -1 and np.isinf(d2[0]) and n[0].tolist() == [0, 0, -1] and bary[0].tolist() == [0, 0]
    n, d2, face, _ = NR.transfer_f32(p, F([[0, 0, -3]]), None, v, f, vn, 0.005, oriented=True)           # ... normalised
    assert face[0] == -1 and n[0].tolist() == [0, 0, -1]
    n, d2, face, _ = NR.transfer_f32(p, m, None, v, f, vn, 0.005, oriented=False)                        # 0.004 is within 0.005
    assert face[0] in (2, 3) and n[0].tolist() == [0, 0, 1]
    for bad_m in ([0, 0, 0], [np.nan, 0, -1], [np.inf, 0, -1], [1e-30, 0, 0]):                             # no direction: no face is eligible, (0, 0, 1)
        n, d2, face, _ = NR.transfer_f32(p, F([bad_m]), None, v, f, vn, 1.0, oriented=True)
        assert face[0] == -1 and n[0].tolist() == [0, 0, 1]
    n, d2, face, _ = NR.transfer_f32(p, m, [0], v, f, vn, 1.0)                                           # not valid: normal 0
    assert face[0] == -1 and np.isinf(d2[0]) and n[0].tolist() == [0, 0, 0]
    n, d2, face, _ = NR.transfer_f32(F([[0.3, np.nan, 0]]), m, None, v, f, vn, 1.0)
    assert face[0] == -1 and n[0].tolist() == [0, 0, 0]
    # the float64 definition says the same
    for oriented, want in ((False, (2, 3)), (True, (0, 1))):
        N, d, face64, _ = NR.transfer_f64(p, m, v, f, vn, 1.0, oriented)
        assert face64[0] in want and abs(d[0] - (0.006 if oriented else 0.004)) < 1e-9 and N[0].tolist() == [0, 0, -1.0 if oriented else 1.0]
    assert NR.transfer_f64(p, m, v, f, vn, 0.005, True)[2][0] == -1


def test_f32_rule_agrees_with_the_float64_definition_on_the_winner():
    """Wherever the best two float64 candidates differ in distance by more than meshdist's E = 33 u M (DR.lower_error), the f32
    rule picks the float64 winner; and its normal is the float64 normal to 1e-5."""
    v, f, vn = NR.lattice()
    g = np.random.RandomState(5)
    p = g.uniform((-1, -1, -0.3), (1, 1, 0.6), (600, 3)).astype(F)
    m = g.normal(size=(600, 3)).astype(F)
    checked = 0
    for oriented in (True, False):
        n32, d2, face, _ = NR.transfer_f32(p, m, None, v, f, vn, 2.0, oriented)
        N, d, face64, dist = NR.transfer_f64(p, m, v, f, vn, 2.0, oriented)
        two = np.sort(dist, 1)[:, :2]
        M = max(np.abs(p).max(), np.abs(v).max())
        sure = np.isfinite(two[:, 0]) & (two[:, 1] - two[:, 0] > DR.lower_error(M))
        assert sure.sum() > 400
        assert np.array_equal(face[sure], face64[sure])
        assert np.abs(np.sqrt(d2[sure].astype(np.float64)) - d[sure]).max() < 1e-6
        assert np.abs(n32[sure].astype(np.float64) - N[sure]).max() < 1e-5
        assert np.array_equal(face < 0, face64 < 0)                                   # nothing is near the reach of 2
        checked += int(sure.sum())
        if oriented:
            assert (face < 0).sum() == 0 and len(set((face // 72).tolist())) == 2     # both sheets win somewhere
    assert checked > 900


# ---- 5. two quality conditions, on the f32 reference


def test_ripple_the_map_recovers_the_relief_a_flat_mesh_lost():
    """The detail is the rippled sheet z = 0.01 sin(2 pi x / 0.25) with its analytic vertex normals; the simplified mesh is the
    flat square z = 0, whose every normal is (0, 0, 1).  The truth for a texel is the analytic normal at the point of the true
    curve nearest to it (Newton's method in float64), which does not know the mesh.  The u8 map read back the way a viewer reads
    it is within a degree of that in the mean -- quantisation alone allows about 0.4 degrees -- and ten times nearer than the flat
    mesh's normals.  A wrong face would be off by up to 28 degrees (two slopes of 14)."""
    v, f, vn = NR.ripple_sheet()
    assert len(f) == 1024 and len(v) == 65 * 9
    g = np.random.RandomState(21)
    p = np.concatenate([g.uniform(0.02, 0.98, (500, 2)), np.zeros((500, 1))], 1).astype(F)
    up = np.tile(F([0, 0, 1]), (500, 1))
    image, (n, d2, face, _) = NR.bake_image(p, -up, np.ones(500, np.uint8), v, f, vn, 0.05)
    assert (face >= 0).all() and np.sqrt(d2.max()) <= 0.0101
    truth = NR.ripple_normal(NR.ripple_foot(p[:, 0].astype(np.float64)))
    err = NR.angles(NR.decode(image), truth)
    flat = NR.angles(up, truth)
    raw = NR.angles(n, truth)
    print("ripple: map mean %.3f max %.3f deg, before quantisation mean %.3f max %.3f, flat normals mean %.3f max %.3f"
          % (err.mean(), err.max(), raw.mean(), raw.max(), flat.mean(), flat.max()))
    assert err.mean() <= 1.0 and err.mean() <= flat.mean() / 10.0
    assert flat.mean() > 5.0


def test_sphere_the_map_of_a_fine_icosphere_on_a_coarse_one():
    """Detail: the icosphere of 3 subdivisions (1 280 faces) with radial normals; simplified: the icosphere of 1 subdivision (80
    faces), sampled at the barycentric lattice T = 6 of every face (2 240 texels) with its own interpolated radial normals.  The
    true normal at a texel is its direction from the centre.  Orientation changes no winner on a convex shape."""
    dv, df, dvn = NR.icosphere(3)
    lv, lf, lvn = NR.icosphere(1)
    assert len(df) == 1280 and len(lf) == 80
    p, m, owner = NR.barycentric_texels(lv, lf, lvn, 6)
    assert len(p) == 2240
    image, (n, d2, face, _) = NR.bake_image(p, -m, np.ones(len(p), np.uint8), dv, df, dvn, 0.5, oriented=True)
    _, d2_u, face_u, _ = NR.transfer_f32(p, m, None, dv, df, dvn, 0.5, oriented=False)
    assert (face >= 0).all() and np.array_equal(face, face_u) and np.array_equal(d2.view(np.int32), d2_u.view(np.int32))
    truth = p.astype(np.float64)
    err, raw = NR.angles(NR.decode(image), truth), NR.angles(n, truth)
    flat = NR.angles(NR.face_normals(lv, lf)[owner], truth)
    print("sphere: map mean %.3f max %.3f deg, before quantisation mean %.3f max %.3f, face normals mean %.3f max %.3f"
          % (err.mean(), err.max(), raw.mean(), raw.max(), flat.mean(), flat.max()))
    assert err.mean() <= 1.0 and err.mean() <= flat.mean() / 10.0 and raw.mean() <= 1.0 and raw.mean() <= flat.mean() / 10.0
    assert flat.mean() > 5.0
