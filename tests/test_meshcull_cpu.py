"""CPU: the C ABI of libngp_meshcull.so (header, exports, ctypes, code object, host-side argument checks), the numpy restatement
the GPU tests compare against (tests/mesh_visibility_reference.py) on the two-shell scene, and the Python API's argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mc_reference as R
from tests import mesh_visibility_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngp_meshcull.h")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


def test_header_compiles_as_c99_alone_and_after_the_other_three():
    for src in ('#include "ngp_meshcull.h"\nint main(void) { return 0; }\n',
                '#include "ngp_hip.h"\n#include "ngp_mesh.h"\n#include "ngp_meshfilter.h"\n#include "ngp_meshcull.h"\n'
                'int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n'):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}


def test_library_exports_exactly_its_header():
    from ngp_pl_amd import _abi, _meshcull_lib
    protos = _abi.parse(HEADER)
    assert len(protos) == 7 and all(n.startswith("ngp_meshcull_") for n in protos)
    assert _exports(_meshcull_lib.LIB_PATH) == set(protos)
    assert set(_meshcull_lib.exported_symbols()) == set(protos)
    lib = _meshcull_lib.lib()
    assert lib.ngp_meshcull_abi_version() == 1 == _meshcull_lib.ABI_VERSION and lib.ngp_meshcull_build_arch() == b"gfx950"


def test_the_four_libraries_share_no_symbol():
    from ngp_pl_amd import _abi, _lib, _mesh_lib, _meshcull_lib, _meshfilter_lib
    for m in (_lib, _mesh_lib, _meshfilter_lib, _meshcull_lib):
        m.lib()
    own = _exports(_meshcull_lib.LIB_PATH)
    others = _exports(_lib.LIB_PATH) | _exports(_mesh_lib.LIB_PATH) | _exports(_meshfilter_lib.LIB_PATH)
    assert own and len(others) > 100
    assert not own & others
    assert not [s for s in others if s.startswith("ngp_meshcull")]
    assert not [s for s in own if not s.startswith("ngp_meshcull_")]
    declared_elsewhere = set(_abi.parse_all())
    for h in ("ngp_mesh.h", "ngp_meshfilter.h"):
        declared_elsewhere |= set(_abi.parse(os.path.join(ROOT, "include", h)))
    assert not set(_abi.parse(HEADER)) & declared_elsewhere


def test_ctypes_agrees_with_the_header():
    from ngp_pl_amd import _abi, _meshcull_lib
    protos = _abi.parse(HEADER)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _meshcull_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    lib = _meshcull_lib.lib()
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        want = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret]
        assert f.restype is want, name


def test_code_object_is_gfx950_only():
    from ngp_pl_amd import _meshcull_lib
    blob = open(_meshcull_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob


def test_argument_validation_needs_no_gpu():
    from ngp_pl_amd import _lib, _meshcull_lib
    lib = _meshcull_lib.lib()
    V, F = 100000, 180000
    ws = lib.ngp_meshcull_workspace_bytes(V, F)
    assert 5 * V <= ws < 5 * V + 12 * ((V + F) // 2048 + 2) + 8 * 256          # 5 B per vertex, 12 B per block, alignment
    assert lib.ngp_meshcull_workspace_bytes(0, 0) > 0
    for v, f in ((-1, 5), (5, -1), (2 ** 31, 5), (5, 2 ** 31)):
        assert lib.ngp_meshcull_workspace_bytes(v, f) == 0
    W, H, cams = 800, 600, 100
    assert lib.ngp_meshcull_zbuffer_bytes(W, H, cams) == 4 * W * H * cams
    assert lib.ngp_meshcull_zbuffer_bytes(16384, 16384, 2 ** 31 - 1) == 4 * 16384 * 16384 * (2 ** 31 - 1)     # 64-bit sizes
    for w, h, c in ((0, H, cams), (W, 0, cams), (16385, H, cams), (W, 16385, cams), (-1, H, cams), (W, H, 0), (W, H, -3), (W, H, 2 ** 31)):
        assert lib.ngp_meshcull_zbuffer_bytes(w, h, c) == 0
    one = 4 * W * H
    fake = C.c_void_p(4096)          # never dereferenced: every call below is rejected before a launch
    big = 2 ** 31

    def views(vertices=fake, faces=fake, n_v=V, n_f=F, K=fake, poses=fake, n_cams=cams, w=W, h=H, zbuf=fake, zbytes=one, out=fake):
        return ("ngp_meshcull_views", vertices, faces, n_v, n_f, K, poses, n_cams, w, h, 0.05, 0.01, zbuf, zbytes, out, None)

    def count(faces=fake, vv=fake, n_v=V, n_f=F, w=fake, wb=ws, totals=fake):
        return ("ngp_meshcull_count", faces, vv, 1, n_v, n_f, w, wb, totals, None)

    def emit(faces=fake, vv=fake, vertices=fake, normals=fake, colors=fake, n_v=V, n_f=F, w=fake, wb=ws, ov=1, of=1, vo=fake, no=fake, co=fake,
             fo=fake):
        return ("ngp_meshcull_emit", faces, vv, 1, vertices, normals, colors, n_v, n_f, w, wb, ov, of, vo, no, co, fo, None)

    bad = [
        views(vertices=None), views(faces=None), views(K=None), views(poses=None), views(zbuf=None), views(out=None),       # nulls
        views(n_v=-1), views(n_f=-1), views(n_cams=0), views(n_cams=-1),                                                     # sizes
        views(w=0), views(h=0), views(w=16385), views(h=16385), views(w=-5),                                                # W / H out of range
        views(zbytes=one - 1), views(zbytes=0),                                                                             # less than one camera
        count(faces=None), count(vv=None), count(w=None), count(totals=None), count(wb=ws - 1), count(n_v=-1), count(n_f=-1),
        emit(faces=None), emit(vv=None), emit(vertices=None), emit(w=None), emit(wb=ws - 1), emit(vo=None), emit(no=None), emit(colors=None),
        emit(fo=None), emit(ov=-1), emit(of=-1), emit(ov=V + 1), emit(of=F + 1), emit(n_v=-1),
    ]
    for args in bad:
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshcull_lib.call(*args)
    too_big = [views(n_v=big), views(n_f=big), views(n_cams=big), count(n_v=big), count(n_f=big), emit(n_v=big), emit(n_f=big)]
    for args in too_big:
        with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
            _meshcull_lib.call(*args)
    # zero-sized meshes and an empty result: nothing to launch
    assert _meshcull_lib.call(*views(vertices=None, faces=None, n_v=0, n_f=0, K=None, poses=None, zbuf=None, zbytes=0, out=None)) == 0
    assert _meshcull_lib.call(*views(vertices=None, faces=None, n_v=0, n_f=5, zbuf=None, out=None)) == 0
    assert _meshcull_lib.call(*count(faces=None, vv=None, n_v=0, n_f=0, w=None, wb=0, totals=None)) == 0
    assert _meshcull_lib.call(*emit(faces=None, vv=None, vertices=None, normals=None, colors=None, n_v=0, n_f=0, w=None, wb=0, ov=0, of=0,
                                    vo=None, no=None, co=None, fo=None)) == 0
    assert _meshcull_lib.call(*emit(normals=None, colors=None, ov=0, of=0, vo=None, no=None, co=None, fo=None)) == 0


def test_python_api_argument_checks():
    import torch
    from ngp_pl_amd import mesh
    v = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    K, poses, wh = torch.eye(3), torch.eye(4)[None, :3].repeat(2, 1, 1), (8, 6)
    fns = (lambda m, K=K, poses=poses, wh=wh: mesh.vertex_views(m, K, poses, wh, 0.1),
           lambda m, K=K, poses=poses, wh=wh: mesh.cull_invisible(m, K, poses, wh, 0.1),
           lambda m, K=K, poses=poses, wh=wh: mesh.cull_invisible(m, K, poses, wh, 0.1, min_views=0))
    for fn in fns:
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(mesh.Mesh(v, f))
        for bad in (f.long(), f.float(), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(6, dtype=torch.int32), f.numpy()):
            with pytest.raises(ValueError):
                fn(mesh.Mesh(v, bad))
        with pytest.raises(ValueError):
            fn(mesh.Mesh(v.double(), f))
        with pytest.raises(ValueError):
            fn(mesh.Mesh(v, f, torch.zeros(5, 3)))
        # the cameras: shapes and the image size, before the device is looked at
        for kw in (dict(K=torch.eye(4)), dict(K=torch.zeros(9)), dict(poses=torch.zeros(3, 4)), dict(poses=torch.zeros(0, 3, 4)),
                   dict(poses=torch.zeros(2, 4, 3)), dict(poses=torch.zeros(2, 2, 4)), dict(wh=(0, 6)), dict(wh=(8, 16385)), dict(wh=(8,)),
                   dict(wh=(8, 6, 3))):
            with pytest.raises(ValueError):
                fn(mesh.Mesh(v, f), **kw)
    # (C, 4, 4) poses and numpy cameras are taken as NGP.mark_invisible_cells takes them: the CPU mesh is what is refused
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.vertex_views(mesh.Mesh(v, f), np.eye(3), np.tile(np.eye(4), (3, 1, 1)), wh, 0.1)


@pytest.fixture(scope="module")
def scene():
    vol = VR.shells_volume()
    v, f, n, _ = R.marching_cubes(vol, 0.0, (0, 0, 0), (1, 1, 1))
    return v, f, n, VR.intrinsics(70, 48, 32), VR.ring_cameras(), (96, 64), 0.05, 2 / 39


def test_restatement_keeps_the_outer_sheet_whole_and_nothing_else(scene):
    """Two concentric shells seen from 14 cameras outside: the outer sheet (r ~ 0.40) is seen, the three sheets behind it (0.30,
    0.20, 0.10) are not."""
    v, f, n, K, poses, wh, near, bias = scene
    assert v.shape == (8688, 3) and f.shape == (17360, 3) and poses.shape == (14, 3, 4)
    zb = VR.zbuffers(v, f, K, poses, wh, near)
    assert zb.shape == (14, 64, 96) and zb.dtype == np.uint32
    depth = zb.view(np.float32)
    hit = zb != VR.INF_BITS
    assert hit.any(axis=(1, 2)).all() and not hit[:, 0, 0].any()               # every camera sees the ball, no corner does
    assert depth[hit].min() > 1.5 - 0.41 and depth[hit].max() < 1.5 + 0.01     # the near half of the outer sphere
    views = VR.vertex_views(v, f, K, poses, wh, bias, near, zb)
    assert views.dtype == np.int32 and np.array_equal(views, VR.vertex_views(v, f, K, poses, wh, bias, near))
    r = np.linalg.norm(v.astype(np.float64) - 0.5, axis=1)
    outer = r > 0.35
    assert outer.sum() == 4632 and (~outer).sum() == 4056
    assert views[outer].min() == 4 and views[outer].max() == 7 and (views[~outer] == 0).all()
    ids = np.repeat(np.arange(len(v), dtype=np.float32)[:, None], 3, 1)        # rides along as "colours": where a vertex came from
    for min_views in (1, 4):
        v1, f1, n1, id1 = VR.cull(v, f, views, min_views, n, ids)
        assert len(v1) == 4632 and R.is_closed_oriented(f1) and R.euler(v1, f1) == 2
        idx = id1[:, 0].astype(np.int64)
        assert np.array_equal(idx, np.nonzero(outer)[0]) and np.array_equal(v[idx], v1) and np.array_equal(n[idx], n1)
        assert np.array_equal(idx[f1], f[outer[f[:, 0]]])                     # the outer sheet's faces, in order, re-indexed
    # a face is kept by ANY of its vertices, and brings all three along
    v5, f5, _, _ = VR.cull(v, f, views, 5)
    keep5 = (views[f] >= 5).any(1)
    assert 0 < keep5.sum() < 9260 and len(f5) == keep5.sum() and len(v5) == len(np.unique(f[keep5])) > (views >= 5).sum()
    v8, f8, _, _ = VR.cull(v, f, views, 8)
    assert v8.shape == (0, 3) and f8.shape == (0, 3)


def test_restatement_edge_rules():
    K = VR.intrinsics(10, 8, 8)
    pose = VR.look_at((0, 0, -2.0), (0, 0, 0), up=(0, -1, 0))
    # a quad at z = 0 (d = 2) covering u, v in [3, 13]; a far vertex behind it; one exactly at u == W; one behind the camera
    v = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [0.05, 0.05, 1], [4.0, 0, 3], [0, 0, -3]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 0, 1], [0, 1, 9], [-1, 1, 2]], np.int32)     # two real, one degenerate, two out of range
    u, vv, d = VR.project(v, K, pose)
    assert d.tolist() == [2, 2, 2, 2, 3, 5, -1] and u[5] == 16 and sorted(set(u[:4].tolist())) == [3, 13]
    zb = VR.zbuffer(v, f, K, pose, (16, 16), 0.05)
    covered = zb != VR.INF_BITS
    # centres i + 0.5 in [3, 13] -> pixels 3..12; both faces write the shared diagonal, the minimum does not care
    want = np.zeros((16, 16), bool)
    want[3:13, 3:13] = True
    assert np.array_equal(covered, want) and (zb.view(np.float32)[covered] == 2).all()
    views = VR.vertex_views(v, f, K, pose[None], (16, 16), 0.25, 0.05)
    assert views.tolist() == [1, 1, 1, 1, 0, 0, 0]        # occluded (3 > 2 + 0.25), on the border u == W, behind the camera
    assert VR.vertex_views(v, f, K, pose[None], (16, 16), 1.0, 0.05).tolist() == [1, 1, 1, 1, 1, 0, 0]      # bias reaches it
    v1, f1, _, _ = VR.cull(v, f, views, 1)
    assert np.array_equal(v1, v[:4]) and f1.tolist() == [[0, 1, 2], [0, 2, 3], [0, 0, 1]]
    # a face across the near plane occludes nothing
    assert not (VR.zbuffer(v, np.array([[0, 1, 6]], np.int32), K, pose, (16, 16), 0.05) != VR.INF_BITS).any()
    # either winding
    assert np.array_equal(VR.zbuffer(v, f[:2, ::-1], K, pose, (16, 16), 0.05), VR.zbuffer(v, f[:2], K, pose, (16, 16), 0.05))
    assert VR.zbuffers(v, f[:0], K, pose[None], (16, 16), 0.05).tolist() == [[[VR.INF_BITS] * 16] * 16]
