"""CPU: the C ABI of libngp_meshtsdf.so (header, exports, ctypes, code object, host-side argument checks), the Python API's
argument checks, and the numpy restatement the GPU tests compare against (tests/mesh_tsdf_reference.py): its edge rules on
hand-worked points, and what the rule is for on the analytic sphere scene (one closed surface where the depth maps say it is)."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from tests import mc_reference as R
from tests import mesh_components_reference as CR
from tests import mesh_tsdf_reference as TR
from tests import mesh_visibility_reference as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ngp_meshtsdf.h")
OTHERS = ("ngp_hip.h", "ngp_mesh.h", "ngp_meshfilter.h", "ngp_meshcull.h", "ngp_meshsimplify.h")


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


def test_header_compiles_as_c99_alone_and_after_the_other_five():
    inc = lambda names: "".join('#include "%s"\n' % n for n in names)
    for src in (inc(["ngp_meshtsdf.h"]) + "int main(void) { return 0; }\n",
                inc(OTHERS + ("ngp_meshtsdf.h",)) + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n",
                inc(("ngp_meshtsdf.h",) + OTHERS[:0:-1]) + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n"):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}
    assert "#ifndef NGP_EINVAL" in text and "#ifndef NGP_ERANGE" in text


def test_library_exports_exactly_its_header():
    from ngp_pl_amd import _abi, _meshtsdf_lib
    protos = _abi.parse(HEADER)
    assert set(protos) == {"ngp_meshtsdf_" + n for n in ("abi_version", "build_arch", "state_bytes", "integrate", "finish")}
    assert _exports(_meshtsdf_lib.LIB_PATH) == set(protos)
    assert set(_meshtsdf_lib.exported_symbols()) == set(protos)
    lib = _meshtsdf_lib.lib()
    assert lib.ngp_meshtsdf_abi_version() == 1 == _meshtsdf_lib.ABI_VERSION and lib.ngp_meshtsdf_build_arch() == b"gfx950"


def test_the_six_libraries_share_no_symbol():
    from ngp_pl_amd import _abi, _lib, _mesh_lib, _meshcull_lib, _meshfilter_lib, _meshsimplify_lib, _meshtsdf_lib
    mods = (_lib, _mesh_lib, _meshfilter_lib, _meshcull_lib, _meshsimplify_lib, _meshtsdf_lib)
    for m in mods:
        m.lib()
    exports = [_exports(m.LIB_PATH) for m in mods]
    assert all(exports) and len(exports[0]) >= 100
    assert len(_abi.parse()) == 100                             # ngp_hip.h stays at its 100 entry points
    for i, a in enumerate(exports):
        for b in exports[i + 1:]:
            assert not a & b
    own, others = exports[-1], set().union(*exports[:-1])
    assert not [s for s in others if s.startswith("ngp_meshtsdf")]
    assert not [s for s in own if not s.startswith("ngp_meshtsdf_")]
    declared_elsewhere = set(_abi.parse_all())
    for h in OTHERS[1:]:
        declared_elsewhere |= set(_abi.parse(os.path.join(ROOT, "include", h)))
    assert not set(_abi.parse(HEADER)) & declared_elsewhere


def test_ctypes_agrees_with_the_header():
    from ngp_pl_amd import _abi, _meshtsdf_lib
    protos = _abi.parse(HEADER)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _meshtsdf_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    lib = _meshtsdf_lib.lib()
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        want = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[pr.ret]
        assert f.restype is want, name


def test_code_object_is_gfx950_only():
    from ngp_pl_amd import _meshtsdf_lib
    blob = open(_meshtsdf_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob


def test_argument_validation_needs_no_gpu():
    from ngp_pl_amd import _lib, _meshtsdf_lib
    from ngp_pl_amd._mesh_lib import bounds6
    lib = _meshtsdf_lib.lib()
    assert lib.ngp_meshtsdf_state_bytes(24, 20, 17) == 12 * 24 * 20 * 17
    assert lib.ngp_meshtsdf_state_bytes(2, 2, 2) == 96
    assert lib.ngp_meshtsdf_state_bytes(4096, 4096, 4096) == 12 * 2 ** 36           # 64-bit sizes, the largest lattice
    for shape in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (-4, 8, 8), (65536, 8, 8), (8, 65536, 8), (8, 8, 65536), (65535, 65535, 17)):
        assert lib.ngp_meshtsdf_state_bytes(*shape) == 0
    fake = C.c_void_p(4096)          # never dereferenced: every call below is rejected before a launch
    b6 = bounds6((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    nan, inf = float("nan"), float("inf")

    def integrate(nx=24, ny=20, nz=17, b=b6, K=fake, poses=fake, depth=fake, n_cams=5, w=96, h=64, near=0.05, trunc=0.1, acc=fake, seen=fake,
                  behind=fake):
        return ("ngp_meshtsdf_integrate", nx, ny, nz, b, K, poses, depth, n_cams, w, h, near, trunc, acc, seen, behind, None)

    def finish(n=1000, acc=fake, seen=fake, behind=fake, vol=fake):
        return ("ngp_meshtsdf_finish", n, acc, seen, behind, vol, None)

    bad = [
        integrate(b=None), integrate(K=None), integrate(poses=None), integrate(depth=None), integrate(acc=None), integrate(seen=None),
        integrate(behind=None),                                                                                                    # nulls
        integrate(nx=1), integrate(ny=0), integrate(nz=-3), integrate(nx=65536), integrate(nx=65535, ny=65535), integrate(n_cams=0),
        integrate(n_cams=-1),                                                                                                      # sizes
        integrate(w=0), integrate(h=0), integrate(w=16385), integrate(h=16385), integrate(w=-5),                                   # W / H out of range
        integrate(trunc=0.0), integrate(trunc=-0.1), integrate(trunc=nan), integrate(trunc=inf), integrate(trunc=-inf),
        integrate(trunc=1e-50),                                                                                                   # 0 as a float
        integrate(b=bounds6((0, 0, 0), (1, 0, 1))), integrate(b=bounds6((0, 0, 0), (1, nan, 1))), integrate(b=bounds6((0, 0, 0), (inf, 1, 1))),
        finish(acc=None), finish(seen=None), finish(behind=None), finish(vol=None), finish(n=-1), finish(n=2 ** 36 + 1),
    ]
    for args in bad:
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshtsdf_lib.call(*args)
    with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
        _meshtsdf_lib.call(*integrate(n_cams=2 ** 31))
    # zero points: nothing to launch
    assert _meshtsdf_lib.call(*finish(n=0, acc=None, seen=None, behind=None, vol=None)) == 0
    assert _meshtsdf_lib.call(*finish(n=0)) == 0


def test_python_api_argument_checks():
    import torch
    from ngp_pl_amd import mesh
    K, poses, wh = torch.eye(3), torch.eye(4)[None, :3].repeat(2, 1, 1), (8, 6)
    depths = torch.ones(2, 6, 8)
    bounds = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))

    def vol(resolution=8, bounds=bounds, K=K, poses=poses, wh=wh, depths=depths, trunc=0.1, **kw):
        return mesh.tsdf_volume(resolution, bounds, K, poses, wh, depths, trunc, **kw)

    with pytest.raises(RuntimeError, match="no CPU path"):
        vol()
    with pytest.raises(RuntimeError, match="no CPU path"):       # (C, 4, 4) poses and numpy cameras are taken: the CPU depths are refused
        vol(K=np.eye(3), poses=np.tile(np.eye(4), (2, 1, 1)), resolution=(8, 9, 10), max_cameras_per_call=1, return_state=True)
    for kw in (dict(K=torch.eye(4)), dict(K=torch.zeros(9)), dict(poses=torch.zeros(3, 4)), dict(poses=torch.zeros(0, 3, 4)),
               dict(poses=torch.zeros(2, 4, 3)), dict(poses=torch.zeros(2, 2, 4)), dict(wh=(0, 6)), dict(wh=(8, 16385)), dict(wh=(8,)),
               dict(wh=(8, 6, 3)),                                                                          # the cameras
               dict(resolution=1), dict(resolution=(8, 8)), dict(resolution=(8, 1, 8)),                     # the lattice
               dict(bounds=((0, 0, 0), (1, 0, 1))), dict(bounds=((0, 0, 0), (1, 1))), dict(bounds=((0, 0, 0), (1, float("inf"), 1))), dict(bounds=None),
               dict(depths=depths.double()), dict(depths=torch.ones(2, 8, 6)), dict(depths=torch.ones(3, 6, 8)), dict(depths=torch.ones(2, 48)),
               dict(depths=depths.numpy()), dict(depths=depths.int()),                                      # the depth maps: (C, H, W) f32
               dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=float("nan")), dict(trunc=float("inf")), dict(trunc=1e-50),
               dict(max_cameras_per_call=0), dict(max_cameras_per_call=-2)):
        with pytest.raises(ValueError):
            vol(**kw)
    cpu_model = types.SimpleNamespace(xyz_min=torch.zeros(1, 3), xyz_max=torch.ones(1, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.render_depths(cpu_model, K, poses, wh)
    for kw in (dict(K=torch.eye(4)), dict(poses=torch.zeros(0, 3, 4)), dict(img_wh=(8, 0))):
        with pytest.raises(ValueError):
            mesh.render_depths(cpu_model, **dict(dict(K=K, poses=poses, img_wh=wh), **kw))
    # extract_mesh(tsdf=...): the options are checked before the model is rendered
    for bad in (dict(K=K, poses=poses, img_wh=wh, trunc_voxels=0.0), dict(K=K, poses=poses, img_wh=wh, trunc_voxels=float("nan")),
                dict(K=torch.eye(4), poses=poses, img_wh=wh)):
        with pytest.raises(ValueError):
            mesh.extract_mesh(cpu_model, 8, tsdf=bad)
    with pytest.raises(TypeError):
        mesh.extract_mesh(cpu_model, 8, tsdf=dict(K=K, poses=poses, img_wh=wh, truncation=3))


def test_restatement_edge_rules():
    """One camera at (0, 0, -2) looking along +z: d = z + 2, u = 10 x / d + 8, v = 10 y / d + 8, 16 x 16 pixels.  The depth
    map is the plane z = 0 (D = 2) with four special pixels in row 8; trunc = 0.5."""
    K = VR.intrinsics(10, 8, 8)
    pose = VR.look_at((0, 0, -2.0), (0, 0, 0), up=(0, -1, 0))[None]
    wh, near, trunc = (16, 16), 0.25, 0.5
    depth = np.full((1, 16, 16), 2.0, np.float32)
    depth[0, 8, 9:13] = [np.nan, 0.0, -1.0, np.inf]
    pts = np.array([
        [0, 0, 0.5],                  # 0: d = 2.5, sdf = -0.5 == -trunc exactly: contributes -1, not behind
        [0, 0, 0.75],                 # 1: sdf = -0.75 < -trunc: behind
        [0, 0, -1.0],                 # 2: d = 1, sdf = 1, q = 2: truncated to 1
        [0, 0, -0.25],                # 3: d = 1.75, sdf = 0.25, q = 0.5
        [0.3, 0.1, 0],                # 4: pixel (9, 8) holds NaN: no observation
        [0.5, 0.1, 0],                # 5: pixel (10, 8) holds 0: no observation
        [0.7, 0.1, 0],                # 6: pixel (11, 8) holds -1: no observation
        [0.9, 0.1, 0],                # 7: pixel (12, 8) holds +inf: sdf = +inf, q = +inf, contributes 1
        [4.0, 0, 3],                  # 8: d = 5, u = 16 == W: outside
        [0, 0, -1.75],                # 9: d = 0.25 == near: inside
        [0, 0, np.nextafter(np.float32(-1.75), np.float32(-2))],     # 10: d just under near: skipped
        [0, 0, -3],                   # 11: behind the camera
    ], np.float32)
    u, v, d = VR.project(pts, K, pose[0])
    assert d[:4].tolist() == [2.5, 2.75, 1, 1.75] and u[8] == 16 and d[9] == 0.25 and 0.2499 < d[10] < 0.25 and d[11] == -1
    assert np.floor(u[4:8]).tolist() == [9, 10, 11, 12] and np.floor(v[4:8]).tolist() == [8, 8, 8, 8]
    acc, seen, behind = TR.integrate(pts, K, pose, wh, depth, near, trunc, TR.clear(len(pts)))
    assert acc.dtype == np.float32 and seen.dtype == np.int32 and behind.dtype == np.int32
    assert seen.tolist() == [1, 0, 1, 1, 0, 0, 0, 1, 0, 1, 0, 0]
    assert behind.tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert acc.tolist() == [-1, 0, 1, 0.5, 0, 0, 0, 1, 0, 1, 0, 0]
    vol = TR.finish((acc, seen, behind))
    assert vol.dtype == np.float32
    #                       at -trunc  hidden  free  near  -- no observation --  inf   u==W  near  under  behind the camera
    assert vol.tolist() == [1, 1, -1, -0.5, -1, -1, -1, -1, -1, -1, -1, -1]
    # a second pass accumulates: the state persists, and two chunks of cameras equal one call
    two = np.concatenate([pose, pose])
    a2, s2, b2 = TR.integrate(pts, K, two, wh, np.concatenate([depth, depth]), near, trunc, TR.clear(len(pts)))
    a1, s1, b1 = TR.integrate(pts, K, pose, wh, depth, near, trunc, (acc.copy(), seen.copy(), behind.copy()))
    assert np.array_equal(a1, a2) and np.array_equal(s1, s2) and np.array_equal(b1, b2)
    assert s2.tolist() == (2 * seen).tolist() and b2.tolist() == (2 * behind).tolist() and np.array_equal(TR.finish((a2, s2, b2)), vol)
    # the lattice is ngp_mesh_lattice_points': lo + i * ((hi - lo) / (n - 1)), x fastest
    lat = TR.lattice((3, 2, 2), ((0, 0, 0), (1, 2, 3)))
    assert lat.dtype == np.float32 and lat.tolist() == [[0, 0, 0], [0.5, 0, 0], [1, 0, 0], [0, 2, 0], [0.5, 2, 0], [1, 2, 0],
                                                        [0, 0, 3], [0.5, 0, 3], [1, 0, 3], [0, 2, 3], [0.5, 2, 3], [1, 2, 3]]


def test_restatement_fuses_the_sphere_into_one_closed_surface():
    """Analytic depth maps of a sphere of radius 0.3 seen from 14 cameras at distance 1.5, 96 x 96, fused on a 48^3 lattice over
    [-0.5, 0.5]^3 with trunc = 4 voxels: one closed component of genus 0, no inner shell, and every vertex near the sphere.

    The distance bound is MEASURED on this restatement, not derived: max | |x| - 0.3 | = 0.641 voxels (median 0.117, V = 3792,
    F = 7580).  The nearest-pixel depth lookup has a silhouette error nobody has computed in closed form; the bound below is that
    measurement plus a quarter voxel for lattice and pixel phase."""
    S = TR.SPHERE
    K, poses, depths = TR.sphere_scene()
    assert poses.shape == (14, 3, 4) and depths.shape == (14, 96, 96) and depths.dtype == np.float32
    hit = np.isfinite(depths)
    assert hit.any(axis=(1, 2)).all() and not hit[:, 0, 0].any() and depths[hit].min() > 1.2 - 1e-3 and depths[hit].max() < 1.5
    acc, seen, behind, vol = TR.tsdf(S["resolution"], S["bounds"], K, poses, S["img_wh"], depths, S["near"], S["trunc"])
    assert vol.shape == (48, 48, 48) and vol.dtype == np.float32
    assert ((seen == 0) & (behind == 0)).sum() == 0                             # every lattice point is in some image
    assert (vol == 1).sum() > 1000 and (vol.reshape(-1)[seen == 0] == 1).all()              # the core was only ever hidden
    assert vol[0, 0, 0] == -1 and vol[24, 24, 24] == 1
    v, f, n, _ = R.marching_cubes(vol, 0.0, *S["bounds"])
    assert len(f) > 5000 and R.is_closed_oriented(f) and R.euler(v, f) == 2
    assert len(np.unique(CR.vertex_labels(f, len(v)))) == 1                    # one component: no inner shell, no floater
    assert R.signed_volume(v, f) > 0                                            # oriented outward
    r = np.linalg.norm(v.astype(np.float64), axis=1)
    assert r.min() > 0.2
    err = np.abs(r - S["radius"]).max() * 47
    print("sphere scene: V=%d F=%d max |r - 0.3| = %.4f voxels, median %.4f" % (len(v), len(f), err, np.median(np.abs(r - 0.3)) * 47))
    assert err <= 0.641 + 0.25, err
    radial = v / r[:, None]
    assert (np.sum(radial * n, 1) > 0).all()                                    # normals point outward: vol falls outward
