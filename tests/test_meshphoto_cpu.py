"""CPU: the C ABI of libngp_meshphoto.so (header, exports, ctypes, code object, build entry, host-side refusals at both edges of
every range), the Python API's, extract_mesh's and the CLI's argument checks, and the numpy restatement the GPU tests compare
against (tests/mesh_photo_reference.py): the boundary cases of THE RULE worked by hand, a fronto-parallel square with an affine
colour reproduced to about a byte, and two parallel squares whose colours the depth test keeps apart exactly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mesh_photo_reference as PR
from tests import mesh_texture_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN = os.path.join(ROOT, "ngp_pl_amd", "csrc", "meshphoto")            # the header lies beside the sources
HEADER = os.path.join(OWN, "ngp_meshphoto.h")
OTHERS = ("ngp_hip.h", "ngp_mesh.h", "ngp_meshfilter.h", "ngp_meshcull.h", "ngp_meshsimplify.h", "ngp_meshtsdf.h", "ngp_meshsmooth.h",
          "ngp_meshtex.h", "ngp_metrics.h", "ngp_meshdist.h", "ngp_meshquadric.h", "ngp_meshdecimate.h")
ATLAS_DIR = os.path.join(ROOT, "ngp_pl_amd", "csrc", "meshatlas")
ENTRY_POINTS = ("abi_version", "build_arch", "accumulate", "resolve")
F = np.float32


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return set(re.findall(r" T (\w+)", out))


# ---- 1. the C ABI


def test_header_compiles_as_c99_alone_and_beside_the_other_headers_in_several_orders():
    assert len(set(OTHERS)) == 12 and set(OTHERS) <= set(os.listdir(os.path.join(ROOT, "include"))) and os.path.exists(HEADER)
    inc = lambda names: "".join('#include "%s"\n' % n for n in names)
    for src in ('#include "ngp_meshphoto.h"\nint main(void) { return 0; }\n',
                inc(OTHERS + ("ngp_meshphoto.h",)) + "int main(void) { return NGP_EINVAL + NGP_ERANGE + NGP_MESHPHOTO_MAX_GUARD + NGP_MESHPHOTO_MAX_POWER; }\n",
                inc(("ngp_meshphoto.h",) + OTHERS[::-1]) + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n",
                inc(OTHERS[5:] + ("ngp_meshphoto.h", "ngp_meshatlas.h") + OTHERS[:5]) + "int main(void) { return NGP_EINVAL + NGP_ERANGE; }\n",
                inc(("ngp_meshatlas.h", "ngp_meshphoto.h")) + "int main(void) { return NGP_MESHATLAS_CLASSES; }\n"):
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                            "-I", OWN, "-I", ATLAS_DIR, "-x", "c", "-"], input=src, text=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        assert r.returncode == 0, r.stdout
    text = open(HEADER).read()
    assert set(re.findall(r"#include\s*[<\"]([^>\"]+)", text)) == {"stddef.h", "stdint.h"}
    assert "#ifndef NGP_EINVAL" in text and "#ifndef NGP_ERANGE" in text and "THE RULE" in text
    from ngp_pl_amd import _meshphoto_lib
    assert "#define NGP_MESHPHOTO_MAX_GUARD %d\n" % _meshphoto_lib.MAX_GUARD in text
    assert "#define NGP_MESHPHOTO_MAX_POWER %d\n" % _meshphoto_lib.MAX_POWER in text


def test_library_exports_exactly_its_header():
    from ngp_pl_amd import _abi, _meshphoto_lib
    protos = _abi.parse(HEADER)
    assert set(protos) == {"ngp_meshphoto_" + n for n in ENTRY_POINTS}
    assert _exports(_meshphoto_lib.LIB_PATH) == set(protos)
    assert set(_meshphoto_lib.exported_symbols()) == set(protos)
    lib = _meshphoto_lib.lib()
    assert lib.ngp_meshphoto_abi_version() == 1 == _meshphoto_lib.ABI_VERSION and lib.ngp_meshphoto_build_arch() == b"gfx950"
    # the argument order the issue of this library set
    assert [p.name for p in protos["ngp_meshphoto_accumulate"].params] == [
        "points", "dirs", "valid", "n", "K", "poses", "n_cams", "W", "H", "images", "zbuf", "near_distance", "bias", "guard", "min_cos", "power",
        "acc", "views", "stream"]
    assert [p.name for p in protos["ngp_meshphoto_resolve"].params] == ["acc", "views", "valid", "n", "min_views", "rgb", "seen", "stream"]


def test_the_fourteen_libraries_share_no_symbol():
    from ngp_pl_amd import (_abi, _lib, _mesh_lib, _meshatlas_lib, _meshcull_lib, _meshdecimate_lib, _meshdist_lib, _meshfilter_lib,
                            _meshphoto_lib, _meshquadric_lib, _meshsimplify_lib, _meshsmooth_lib, _meshtex_lib, _meshtsdf_lib, _metrics_lib)
    mods = (_lib, _mesh_lib, _meshfilter_lib, _meshcull_lib, _meshsimplify_lib, _meshtsdf_lib, _meshsmooth_lib, _meshtex_lib, _metrics_lib,
            _meshdist_lib, _meshquadric_lib, _meshdecimate_lib, _meshatlas_lib, _meshphoto_lib)
    assert len({m.LIB_PATH for m in mods}) == 14
    exports = [_exports(m.LIB_PATH) for m in mods]
    assert all(exports)
    for i, a in enumerate(exports):
        for b in exports[i + 1:]:
            assert not a & b
    own, others = exports[-1], set().union(*exports[:-1])
    assert not [s for s in others if s.startswith("ngp_meshphoto")]
    assert not [s for s in own if not s.startswith("ngp_meshphoto_")]
    declared = set(_abi.parse(HEADER))
    for h in [os.path.join(ROOT, "include", h) for h in OTHERS] + [os.path.join(ATLAS_DIR, "ngp_meshatlas.h")]:
        assert not declared & set(_abi.parse(h)), h


def test_ctypes_agrees_with_the_header():
    from ngp_pl_amd import _abi, _meshphoto_lib
    protos = _abi.parse(HEADER)
    problems = [m for m in (_abi.ctypes_agrees(a, protos[n]) for n, a in _meshphoto_lib._PROTOS.items()) if m]
    assert not problems, "\n".join(problems)
    lib = _meshphoto_lib.lib()
    for name, pr in protos.items():
        f = getattr(lib, name)
        assert f.argtypes is not None and _abi.ctypes_agrees(list(f.argtypes), pr) is None, name
        want = {"int": C.c_int, "const char*": C.c_char_p}[pr.ret]
        assert f.restype is want, name


def test_code_object_is_gfx950_only():
    from ngp_pl_amd import _meshphoto_lib
    blob = open(_meshphoto_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob and b"gfx942" not in blob and b"sm_" not in blob
    for kernel in (b"photo_accumulate", b"photo_resolve"):
        assert kernel in blob


def test_build_links_the_fourteenth_library_with_contraction_off():
    from ngp_pl_amd import _meshphoto_lib, build
    assert build.MESHPHOTO_LIB == _meshphoto_lib.LIB_PATH and build.MESHPHOTO_CFLAGS == ["-ffp-contract=off"]
    assert build.ARCH == "gfx950" and build.MESHPHOTO_SOURCES == [os.path.join("meshphoto", "meshphoto.hip")]
    for rel in build.MESHPHOTO_SOURCES + build.MESHPHOTO_HEADERS:
        assert os.path.exists(os.path.join(build.CSRC, rel)), rel
    # no other library's ABI header or source is compiled into this one (only the shared camera device code and the host helpers
    # every mesh library shares), and the tile size the tests straddle is the kernel's
    source = open(os.path.join(build.CSRC, build.MESHPHOTO_SOURCES[0])).read()
    assert set(re.findall(r'#include\s*"([^"]+)"', source)) == {"ngp_meshphoto.h", "../mesh_camera.h", "../mesh_host.h"}
    assert "constexpr int CAM_TILE = %d;" % _meshphoto_lib.CAM_TILE in source and PR.CAM_TILE == _meshphoto_lib.CAM_TILE


# ---- 2. host refusals at both edges of every range, no GPU


def test_argument_validation_needs_no_gpu():
    """A refused call never launches; an accepted one is made with n == 0, which launches nothing either (the scalar arguments
    are checked first), so both edges of every range are exercised without a GPU."""
    from ngp_pl_amd import _lib, _meshphoto_lib
    fake = C.c_void_p(4096)          # never dereferenced
    up = lambda x: float(np.nextafter(F(x), F(np.inf)))
    down = lambda x: float(np.nextafter(F(x), F(-np.inf)))
    nan, inf, fmax = float("nan"), float("inf"), float(np.finfo(F).max)

    def accumulate(points=fake, dirs=fake, valid=fake, n=100, K=fake, poses=fake, n_cams=3, W=8, H=6, images=fake, zbuf=fake, near=0.01, bias=0.1,
                   guard=1, min_cos=0.1, power=2, acc=fake, views=fake):
        return ("ngp_meshphoto_accumulate", points, dirs, valid, n, K, poses, n_cams, W, H, images, zbuf, near, bias, guard, min_cos, power, acc,
                views, None)

    def resolve(acc=fake, views=fake, valid=fake, n=100, min_views=1, rgb=fake, seen=fake):
        return ("ngp_meshphoto_resolve", acc, views, valid, n, min_views, rgb, seen, None)

    inside = [dict(W=1), dict(W=16384), dict(H=1), dict(H=16384), dict(n_cams=1), dict(n_cams=2 ** 31 - 1), dict(guard=0), dict(guard=4),
              dict(power=1), dict(power=8), dict(min_cos=up(0.0)), dict(min_cos=1.0), dict(bias=0.0), dict(bias=fmax), dict(near=-fmax),
              dict(near=fmax), dict(near=0.0)]
    outside = [dict(W=0), dict(W=16385), dict(H=0), dict(H=16385), dict(W=-1), dict(n_cams=0), dict(n_cams=-1), dict(guard=-1), dict(guard=5),
               dict(power=0), dict(power=9), dict(min_cos=0.0), dict(min_cos=up(1.0)), dict(min_cos=-0.5), dict(min_cos=nan), dict(bias=down(0.0)),
               dict(bias=inf), dict(bias=nan), dict(bias=-1.0), dict(near=inf), dict(near=-inf), dict(near=nan)]
    for kw in inside:
        assert _meshphoto_lib.call(*accumulate(n=0, **kw)) == 0, kw
    for kw in outside:
        for n in (0, 100):           # refused whether or not there is anything to do
            with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
                _meshphoto_lib.call(*accumulate(n=n, **kw))
    for name in ("points", "dirs", "valid", "K", "poses", "images", "zbuf", "acc", "views"):
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshphoto_lib.call(*accumulate(**{name: None}))
        assert _meshphoto_lib.call(*accumulate(n=0, **{name: None})) == 0          # n == 0: the pointers are not looked at
    for kw in (dict(n=-1), dict(acc=C.c_void_p(4100)), dict(acc=C.c_void_p(4104)), dict(zbuf=C.c_void_p(4098)), dict(views=C.c_void_p(4097))):
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshphoto_lib.call(*accumulate(**kw))
    for kw in (dict(n=2 ** 31), dict(n_cams=2 ** 31)):
        with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
            _meshphoto_lib.call(*accumulate(**kw))
    for mv in (1, 2 ** 31 - 1):
        assert _meshphoto_lib.call(*resolve(n=0, min_views=mv)) == 0
    for kw in (dict(min_views=0), dict(min_views=-1), dict(n=-1), dict(min_views=0, n=0), dict(acc=C.c_void_p(4100))):
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshphoto_lib.call(*resolve(**kw))
    for name in ("acc", "views", "valid", "rgb", "seen"):
        with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
            _meshphoto_lib.call(*resolve(**{name: None}))
        assert _meshphoto_lib.call(*resolve(n=0, **{name: None})) == 0
    with pytest.raises(_lib.NgpError, match="NGP_ERANGE"):
        _meshphoto_lib.call(*resolve(n=2 ** 31))


# ---- 3. the Python API's checks, extract_mesh's option parsing and the CLI


def _camera_args(n_cams=2, wh=(8, 6)):
    K = np.array([[8, 0, 4], [0, 8, 3], [0, 0, 1]], F)
    poses = np.tile(PR.IDENTITY[None], (n_cams, 1, 1))
    return dict(images=np.zeros((n_cams, wh[1], wh[0], 3), np.uint8), K=K, poses=poses, img_wh=wh)


def test_python_api_argument_checks():
    import torch
    from ngp_pl_amd import mesh
    v = torch.zeros(4, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    m = mesh.Mesh(v, f, torch.zeros(4, 3))
    cam = _camera_args()
    pts = dict(points=torch.zeros(5, 3), dirs=torch.zeros(5, 3), valid=torch.ones(5, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.photo_colors(m, **pts, **cam, bias=0.1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.bake_texture_from_images(m, **cam, bias=0.1, box=((0, 0, 0), (1, 1, 1)))
    bad = [dict(bias=-0.1), dict(bias=float("inf")), dict(bias=float("nan")), dict(bias="1"), dict(bias=None), dict(bias=True),
           dict(guard=-1), dict(guard=5), dict(guard=1.0), dict(guard=True), dict(min_cos=0), dict(min_cos=0.0), dict(min_cos=1.5), dict(min_cos=float("nan")),
           dict(min_cos=None), dict(power=0), dict(power=9), dict(power=2.0), dict(min_views=0), dict(min_views=1.5), dict(min_views=2 ** 31)]
    for kw in bad:
        with pytest.raises(ValueError, match=list(kw)[0]):
            mesh.photo_colors(m, **pts, **cam, **{"bias": 0.1, **kw})
        with pytest.raises(ValueError, match=list(kw)[0]):
            mesh.bake_texture_from_images(m, **cam, box=((0, 0, 0), (1, 1, 1)), **{"bias": 0.1, **kw})
        if kw != dict(bias=None):                       # extract_mesh's bias=None is twice the lattice spacing
            with pytest.raises(ValueError):
                mesh.extract_mesh(None, 8, texture=dict(texels=2, images=dict(cam, **kw)))
    for near in (float("inf"), float("nan"), "0"):
        with pytest.raises(ValueError, match="near"):
            mesh.photo_colors(m, **pts, **cam, bias=0.1, near=near)
    with pytest.raises(ValueError, match="bias must be given"):
        mesh.bake_texture_from_images(m, **cam, box=((0, 0, 0), (1, 1, 1)))
    with pytest.raises(ValueError, match="exclude"):
        mesh.bake_texture_from_images(m, **cam, bias=0.1, model=object(), fill=(1, 0, 1))
    with pytest.raises(ValueError, match="box"):
        mesh.bake_texture_from_images(m, **cam, bias=0.1, fill=(1, 0, 1))
    for fill in ((1, 0), (1, 0, 2), (-0.1, 0, 0), "abc", 1.0, (float("nan"), 0, 0)):
        with pytest.raises(ValueError, match="fill"):
            mesh.bake_texture_from_images(m, **cam, bias=0.1, fill=fill, box=((0, 0, 0), (1, 1, 1)))
    for chunk in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="chunk"):
            mesh.bake_texture_from_images(m, **cam, bias=0.1, box=((0, 0, 0), (1, 1, 1)), chunk=chunk)
    # the arguments are returned as the f32 values the library will see
    assert mesh._photo_args(0.1, 4, 1, 8, 1, 0.01) == (float(F(0.1)), 4, 1.0, 8, 1, float(F(0.01)))
    assert mesh._photo_args(0, 0, 1e-30, 1, 2 ** 31 - 1, -5)[:5] == (0.0, 0, float(F(1e-30)), 1, 2 ** 31 - 1)
    # the photographs: one (H, W, 3) uint8 per pose
    assert tuple(mesh._photo_images(cam["images"], 2, 8, 6).shape) == (2, 6, 8, 3)
    for images in (cam["images"][:1], cam["images"].astype(np.float32), cam["images"][..., :2], cam["images"].transpose(0, 2, 1, 3), None, [1, 2]):
        with pytest.raises(ValueError, match="images"):
            mesh._photo_images(images, 2, 8, 6)


def test_extract_mesh_texture_options_with_images():
    from ngp_pl_amd import mesh
    cam = _camera_args()
    full = dict(bias=None, guard=1, min_cos=0.1, power=2, min_views=1)
    # without images nothing changes: the int, or the adaptive dict, as before
    assert mesh._texture_options(None) is None and mesh._texture_options(4) == 4 and mesh._texture_options(dict(texels=4)) == 4
    assert mesh._texture_options(dict(texels=4, images=None)) == 4
    assert mesh._texture_options(dict(texel_size=2.0)) == dict(min_texels=1, max_texels=256, texel_size=2.0)
    out = mesh._texture_options(dict(texels=2, images=cam))
    assert set(out) == {"texels", "images"} and out["texels"] == 2
    assert {k: out["images"][k] for k in full} == full and out["images"]["img_wh"] == (8, 6) and out["images"]["images"] is cam["images"]
    out = mesh._texture_options(dict(images=dict(cam, bias=0.5, guard=0, min_cos=1, power=8, min_views=3)))
    assert out["texels"] == 8 and {k: out["images"][k] for k in full} == dict(bias=0.5, guard=0, min_cos=1, power=8, min_views=3)
    out = mesh._texture_options(dict(texel_size=2.0, max_texels=64, images=cam))
    assert {k: v for k, v in out.items() if k != "images"} == dict(min_texels=1, max_texels=64, texel_size=2.0) and out["images"]["guard"] == 1
    out = mesh._texture_options(dict(max_side=512, images=cam))
    assert out["max_side"] == 512 and "images" in out
    less = lambda key: {k: v for k, v in cam.items() if k != key}
    for images in (cam["images"], 3, "x.npz", dict(cam, near=0.1), dict(cam, fill=(1, 0, 1)), less("images"), less("K"), less("poses"), less("img_wh"),
                   dict(cam, images=cam["images"][:1]), dict(cam, img_wh=(6, 8)), dict(cam, K=np.eye(4)), dict(cam, poses=cam["poses"][0]),
                   dict(cam, img_wh=(0, 6)), dict(cam, guard=7)):
        with pytest.raises(ValueError):
            mesh.extract_mesh(None, 8, texture=dict(texels=2, images=images))
    for texture in (dict(texels=0, images=cam), dict(texel_size=1.0, texels=8, images=cam), dict(texels=2, images=cam, border=1), dict(min_texels=2, images=cam)):
        with pytest.raises(ValueError):
            mesh.extract_mesh(None, 8, texture=texture)


def test_cli_lists_the_options_and_refuses_bad_combinations(capsys):
    from ngp_pl_amd import mesh
    with pytest.raises(SystemExit) as e:
        mesh.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for flag in ("--texture-images FILE.npz", "--texture-image-bias B", "--texture-image-guard G", "--texture-image-min-cos C",
                 "--texture-image-power P", "--texture-image-min-views N"):
        assert flag in out
    for bad in (["--out", "y.obj", "--texture-images", "p.npz"],                                    # no atlas option
                ["--out", "y.ply", "--texture-images", "p.npz"],
                ["--out", "y.ply", "--texture-images", "p.npz", "--texture-texels", "2"],               # a PLY carries no texture
                ["--out", "y.ply", "--texture-images", "p.npz", "--texture-texel-size", "1"],
                ["--out", "y.obj", "--texture-texels", "2", "--texture-image-guard", "1"],              # the sub-options need --texture-images
                ["--out", "y.obj", "--texture-texels", "2", "--texture-image-bias", "0.1"],
                ["--out", "y.obj", "--texture-texels", "2", "--texture-image-min-cos", "0.2"],
                ["--out", "y.obj", "--texture-texels", "2", "--texture-image-power", "2"],
                ["--out", "y.obj", "--texture-texels", "2", "--texture-image-min-views", "2"],
                ["--out", "y.obj", "--texture-texels", "2", "--texture-images", "p.npz", "--texture-image-guard", "5"],
                ["--out", "y.obj", "--texture-texels", "2", "--texture-images", "p.npz", "--texture-image-guard", "-1"],
                ["--out", "y.obj", "--texture-texels", "2", "--texture-images", "p.npz", "--texture-image-bias", "-1"],
                ["--out", "y.obj", "--texture-texels", "2", "--texture-images", "p.npz", "--texture-image-bias", "nan"],
                ["--out", "y.obj", "--texture-texels", "2", "--texture-images", "p.npz", "--texture-image-min-cos", "0"],
                ["--out", "y.obj", "--texture-texels", "2", "--texture-images", "p.npz", "--texture-image-min-cos", "1.5"],
                ["--out", "y.obj", "--texture-texels", "2", "--texture-images", "p.npz", "--texture-image-power", "0"],
                ["--out", "y.obj", "--texture-texels", "2", "--texture-images", "p.npz", "--texture-image-power", "9"],
                ["--out", "y.obj", "--texture-max-side", "64", "--texture-images", "p.npz", "--texture-image-min-views", "0"]):
        with pytest.raises(SystemExit) as e:
            mesh.main(["--ckpt", "x"] + bad)
        assert e.value.code == 2, bad
        assert "--texture-" in capsys.readouterr().err


# ---- 4. the restatement on hand-worked cases


@pytest.mark.parametrize("case", PR.hand_cases(), ids=lambda c: c["name"])
def test_hand_worked_cases(case):
    """One point, one camera at the origin with R = I, a 4 x 4 photograph with byte 10 i + 40 j + k: the sample is taken or not as
    the case says, and where it is, acc is w * col and w with the weight and the colour written out here."""
    acc, views = PR.run_case(case)
    assert views.tolist() == [1 if case["accepted"] else 0]
    if not case["accepted"]:
        assert not acc.any()
        assert PR.resolve(acc, views, case["valid"], 1)[1].tolist() == [0]
        return
    x, g = case["points"][0], case["dirs"][0]
    L = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])              # o = 0: e = -x
    cs = -((g[0] * -x[0] + g[1] * -x[1]) + g[2] * -x[2]) / L
    w = cs
    for _ in range(case["power"] - 1):
        w = w * cs
    assert acc.dtype == F and w.dtype == F and acc[0, 3] == w
    if case["name"].startswith("power"):
        assert float(w) == 0.5 ** case["power"]
    if case["col"] is not None:
        assert [acc[0, k] == w * F(case["col"][k]) for k in range(3)] == [True] * 3
        rgb, seen = PR.resolve(acc, views, case["valid"], 1)
        assert seen.tolist() == [1] and PR.quantise(rgb)[0].tolist() == list(case["col"])
        assert PR.resolve(acc, views, case["valid"], 2)[1].tolist() == [0] and PR.resolve(acc, views, [0], 1)[1].tolist() == [0]


def test_hand_cases_cover_the_list():
    names = " | ".join(c["name"] for c in PR.hand_cases())
    for part in ("fx == 0", "u == 0.5", "ulp below 0.5", "u == W - 0.5", "ulp above W - 0.5", "d == near", "ulp below near", "d == z + bias",
                 "ulp above z + bias", "z == d + bias", "cs == min_cos", "empty pixel in the window", "clipped at the corner"):
        assert part in names, part
    # every pair of neighbours differs only in the boundary it sits on: the accepted and the refused side of each
    assert sum(c["accepted"] for c in PR.hand_cases()) >= 12 and sum(not c["accepted"] for c in PR.hand_cases()) >= 12


def test_skipped_points_and_carried_sums():
    """valid == 0, a coordinate or a direction that is not finite: the point keeps the sums it came with; a NaN pose and a pose of
    1e30 read nothing and leave the other cameras alone; cameras in two calls with carried sums equal one call."""
    s = PR.random_scene(65, (16, 12), 5, seed=7)
    base_acc, base_views = PR.accumulate(**s)
    assert 0 < (base_views > 0).sum() < 65 and base_views.max() > 1
    pts, dirs = s["points"].copy(), s["dirs"].copy()
    live = np.nonzero(base_views > 0)[0]
    pts[live[0], 1], pts[live[1], 0], dirs[live[2], 2], dirs[live[3], 0] = np.nan, np.inf, np.nan, -np.inf
    valid = s["valid"].copy()
    valid[live[4]] = 0
    acc0 = np.random.RandomState(0).rand(65, 4).astype(F)
    views0 = np.arange(65, dtype=np.int32)
    acc, views = PR.accumulate(**{**s, "points": pts, "dirs": dirs, "valid": valid}, acc=acc0, views=views0)
    for k in live[:5]:
        assert np.array_equal(acc[k], acc0[k]) and views[k] == views0[k]
    assert (views[live[5:]] > views0[live[5:]]).all()
    poses = s["poses"].copy()
    poses[1] = np.nan
    poses[3, :, 3] = 1e30
    acc_b, views_b = PR.accumulate(**{**s, "poses": poses})
    keep = [0, 2, 4]
    acc_k, views_k = PR.accumulate(**{**s, "poses": s["poses"][keep], "images": s["images"][keep], "zbuf": s["zbuf"][keep]})
    assert np.array_equal(PR.words(acc_b), PR.words(acc_k)) and np.array_equal(views_b, views_k)
    a1, v1 = PR.accumulate(**{**s, "poses": s["poses"][:2], "images": s["images"][:2], "zbuf": s["zbuf"][:2]})
    a2, v2 = PR.accumulate(**{**s, "poses": s["poses"][2:], "images": s["images"][2:], "zbuf": s["zbuf"][2:]}, acc=a1, views=v1)
    assert np.array_equal(PR.words(a2), PR.words(base_acc)) and np.array_equal(v2, base_views)


# ---- 5. a fronto-parallel square with an affine colour


def test_linear_colour_on_a_fronto_parallel_square_within_a_byte():
    """The square lies in the plane z = 0 and every camera looks straight down at it, so screen position is an affine function of
    the position in the plane, and a colour affine in position is affine in (u, v).  The photographs hold, at every pixel centre,
    255 lin rounded to a byte: the exact value plus an error of at most half a byte.  Bilinear interpolation reproduces an affine
    function exactly inside the grid of pixel centres, which is where test 2 of the rule keeps the footprint, so a sample is
    255 lin(x) plus a convex combination of those errors: at most half a byte off.  The blend over the cameras is a convex
    combination of the samples (the weights are positive) and is at most half a byte off as well.  Writing the result as a byte
    adds the other half.  What is left is f32: u and v carry a few ulp of about 40 pixels (1e-5 pixel) at a colour slope of at
    most 6 bytes per pixel, and the dozen roundings of sample, sum and quotient are each 6e-8 of at most 255: under 1e-3 byte
    together.  Hence |byte - 255 lin(x)| <= 1 + 1e-3 for every texel the photographs colour, with x the texel's own point."""
    K, poses, images, zbuf = PR.fronto_scene()
    img_wh = (images.shape[2], images.shape[1])
    nrm = np.tile(F([[0, 0, 1]]), (4, 1))
    p, d, valid = TR.texel_points(PR.SQUARE_V, PR.SQUARE_F, nrm, 24, ((-2, -2, -2), (2, 2, 2)))
    assert (d[valid == 1] == F([0, 0, -1])).all()
    worst = 0.0
    for cams in ([0], [0, 1, 2, 3], [2, 3]):
        rgb, seen, views = PR.photo_colors(None, None, p, d, valid, images[cams], K, poses[cams], img_wh, bias=0.05, zbuf=zbuf[cams])
        seen = seen == 1
        on_square = (valid == 1) & (np.abs(p[:, :2]) < 0.75).all(1)
        assert seen[on_square].all() and views[on_square].min() == len(cams) and not seen[valid == 0].any()
        off = (valid == 1) & (np.abs(p[:, :2]) > 1.0).any(1)            # the extrapolated border of the faces along the square's edge
        assert off.any() and not seen[off].any()
        err = np.abs(PR.quantise(rgb)[seen].astype(np.float64) - 255.0 * PR.lin(p[seen])).max()
        print("cameras %r: %d texels seen, largest error %.4f bytes" % (cams, seen.sum(), err))
        worst = max(worst, err)
        assert err <= 1.0 + 1e-3
    assert worst > 0.5                                   # the bound is not slack by more than a factor of two


# ---- 6. two parallel squares: the depth test keeps their colours apart


def _two_squares(bias, guard=1):
    K, poses, images, zbuf, face = PR.two_squares_scene()
    img_wh = (images.shape[2], images.shape[1])
    p, d, valid = TR.texel_points(PR.TWO_V, PR.TWO_F, PR.TWO_N, PR.TWO_TEXELS, PR.TWO_BOX)
    owner = TR.owners(len(PR.TWO_F), PR.TWO_TEXELS)[0]
    rgb, seen, views = PR.photo_colors(None, None, p, d, valid, images, K, poses, img_wh, bias=bias, guard=guard, zbuf=zbuf)
    centre = PR.centre_pixel_face(p, K, poses, img_wh, face)
    return p, valid == 1, owner, PR.quantise(rgb), seen == 1, views, centre


def test_two_parallel_squares_keep_their_colours():
    """A rear square and a smaller front square a gap of ten times the bias in front of it, photographed head-on and from two
    sides.  Photographs and depth buffers come from one raster (the coverage rule of the cull), so a pixel whose depth is within
    the bias of a rear texel's depth IS a pixel of the rear square, and with guard = 1 the window holds the whole bilinear
    footprint.  Exactly, with no texel exempted: every rear texel the photographs colour has the rear colour; every rear texel
    whose own pixel shows something else in every camera stays unseen.  With the bias as large as the gap both fail."""
    p, valid, owner, byte, seen, views, centre = _two_squares(PR.TWO_BIAS)
    rear, front = valid & (owner < 2), valid & (owner >= 2)
    assert (rear & seen).sum() >= 300 and (front & seen).sum() >= 300       # of 812 texels each, the faces' borders and the shadow included
    assert (byte[rear & seen] == PR.REAR_RGB).all()
    assert (byte[front & seen] == PR.FRONT_RGB).all()
    assert not byte[~seen].any() and not seen[~valid].any()
    hidden = rear & ~np.isin(centre, (0, 1)).any(0)      # in no camera does the texel's own pixel show the rear square
    behind_front = rear & np.isin(centre, (2, 3)).all(0)
    assert behind_front.sum() >= 10 and hidden.sum() > behind_front.sum()
    assert not seen[hidden].any()
    # the part of the rear square that only the oblique cameras see past the front square is coloured, and by fewer cameras
    shadow = rear & np.isin(centre[0], (2, 3))
    assert (shadow & seen).sum() >= 10 and views[shadow & seen].max() <= 2 and views[rear & seen].max() == 3
    # the depth test is what does the work: a bias as large as the gap lets the front square's colour onto the rear one
    p, valid, owner, byte2, seen2, _, _ = _two_squares(PR.GAP)
    mixed = rear & seen2 & (byte2 != PR.REAR_RGB).any(1)
    assert mixed.sum() >= 10 and seen2[behind_front].any()
