"""GPU: libngp_meshphoto.so against the numpy restatement (tests/mesh_photo_reference.py), bit for bit: acc and rgb as int32 words,
views and seen, on the smallest inputs at which each mechanism can fail -- point counts round the wave and the block, W != H,
camera counts round the LDS tile, the boundary cases worked by hand, guard windows larger than the image, every power, points and
poses that are not finite, cameras and points split into chunks with carried sums.  Then photo_colors, bake_texture_from_images,
extract_mesh and the CLI.  Nothing here has a tolerance."""
import json
import os

import numpy as np
import pytest
import torch

from tests import mesh_atlas_reference as AR
from tests import mesh_photo_reference as PR
from tests import mesh_texture_reference as TR
from tests.test_meshtex_gpu import bits, make_model, same_mesh, to_mesh, true_density  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
TILE = PR.CAM_TILE


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def lib_accumulate(s, acc=None, views=None, cams=slice(None), pts=slice(None)):
    """ngp_meshphoto_accumulate on the scene dict `s` (the cameras `cams`, the points `pts`) -> acc, views as device tensors."""
    from ngp_pl_amd import _meshphoto_lib as L
    points, dirs, valid = dev(s["points"][pts]), dev(s["dirs"][pts]), dev(s["valid"][pts])
    poses, images = dev(np.asarray(s["poses"], F)[cams]), dev(s["images"][cams])
    zbuf = dev(np.ascontiguousarray(s["zbuf"][cams]).view(np.int32))
    K = dev(np.asarray(s["K"], F))
    n, W, H = points.shape[0], s["img_wh"][0], s["img_wh"][1]
    acc = torch.zeros(n, 4, device="cuda") if acc is None else acc
    views = torch.zeros(n, dtype=torch.int32, device="cuda") if views is None else views
    L.call("ngp_meshphoto_accumulate", L.ptr(points), L.ptr(dirs), L.ptr(valid), n, L.ptr(K), L.ptr(poses), poses.shape[0], W, H, L.ptr(images),
           L.ptr(zbuf), float(s["near"]), float(s["bias"]), int(s["guard"]), float(s["min_cos"]), int(s["power"]), L.ptr(acc), L.ptr(views), L.stream())
    return acc, views


def lib_resolve(acc, views, valid, min_views=1):
    from ngp_pl_amd import _meshphoto_lib as L
    n = acc.shape[0]
    valid = dev(valid)
    rgb = torch.full((n, 3), -7.0, device="cuda")
    seen = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    L.call("ngp_meshphoto_resolve", L.ptr(acc), L.ptr(views), L.ptr(valid), n, int(min_views), L.ptr(rgb), L.ptr(seen), L.stream())
    return rgb, seen


def check(s, min_views=1, expect_some=True):
    """The library on the scene against the restatement: acc, views, rgb, seen, all bits."""
    want_acc, want_views = PR.accumulate(**s)
    acc, views = lib_accumulate(s)
    assert np.array_equal(bits(acc), PR.words(want_acc)) and np.array_equal(views.cpu().numpy(), want_views)
    for mv in {1, min_views}:
        want_rgb, want_seen = PR.resolve(want_acc, want_views, s["valid"], mv)
        rgb, seen = lib_resolve(acc, views, s["valid"], mv)
        assert np.array_equal(bits(rgb), PR.words(want_rgb)) and np.array_equal(seen.cpu().numpy(), want_seen)
    if expect_some:
        assert want_views.sum() > 0
    return want_acc, want_views


# ---- 1. sizes: points round the wave and the block, W != H, cameras round the LDS tile

SIZES = [1, 63, 64, 65, 255, 256, 257]
CAMERAS = [1, 2, TILE - 1, TILE, TILE + 1]


@pytest.mark.parametrize("k,n", list(enumerate(SIZES)))
def test_point_counts(k, n):
    img_wh, n_cams = ((5, 7), (16, 12))[k % 2], (3, 2, 5)[k % 3]
    check(PR.random_scene(n, img_wh, n_cams, seed=10 + n), min_views=2, expect_some=n > 1)


@pytest.mark.parametrize("img_wh", [(5, 7), (16, 12)])
@pytest.mark.parametrize("n_cams", CAMERAS)
def test_camera_counts_round_the_lds_tile(n_cams, img_wh):
    _, views = check(PR.random_scene(257, img_wh, n_cams, seed=100 + n_cams), min_views=2)
    if n_cams >= TILE - 1:
        assert views.max() > 20                         # the sums really run over tens of cameras


def test_one_point_is_seen():
    s = PR.random_scene(1, (16, 12), 2, seed=1)
    s["points"][:], s["dirs"][:], s["valid"][:] = (0.1, -0.2, 0.0), (0, 0, -1), 1
    _, views = check(s)
    assert views.tolist() == [2]


# ---- 2. the boundary cases worked by hand


def test_hand_worked_cases_through_the_library():
    for case in PR.hand_cases():
        acc, views = lib_accumulate(case)
        want_acc, want_views = PR.run_case(case)
        assert views.tolist() == [1 if case["accepted"] else 0] == want_views.tolist(), case["name"]
        assert np.array_equal(bits(acc), PR.words(want_acc)), case["name"]
        rgb, seen = lib_resolve(acc, views, case["valid"])
        want_rgb, want_seen = PR.resolve(want_acc, want_views, case["valid"], 1)
        assert np.array_equal(bits(rgb), PR.words(want_rgb)) and seen.tolist() == want_seen.tolist() == [int(case["accepted"])], case["name"]
        if case["col"] is not None:
            assert PR.quantise(rgb.cpu().numpy())[0].tolist() == list(case["col"]), case["name"]


# ---- 3. guard, power, min_cos, near


@pytest.mark.parametrize("guard", [0, 1, 4])
def test_guard_window_larger_than_the_image(guard):
    s = PR.random_scene(257, (5, 7), 3, seed=40, bias=0.6, extent=3.0)          # 2 * 4 + 1 = 9 pixels: wider and higher than the photograph
    s["guard"] = guard
    _, views = check(s)
    s["guard"] = 0
    assert views.sum() <= PR.accumulate(**s)[1].sum()    # a larger window only rejects more


@pytest.mark.parametrize("power", [1, 2, 8])
def test_power(power):
    s = PR.random_scene(65, (16, 12), 3, seed=50)
    s["power"] = power
    check(s)


def test_min_cos_and_near_and_bias():
    for kw in (dict(min_cos=1.0), dict(min_cos=0.9), dict(min_cos=1e-6), dict(near=2.5), dict(near=-1.0), dict(bias=0.0), dict(bias=1e30)):
        s = PR.random_scene(129, (16, 12), 3, seed=60)
        s.update(kw)
        check(s, expect_some=False)


# ---- 4. points and poses that are not finite


def test_bad_points_keep_their_sums():
    s = PR.random_scene(130, (16, 12), 3, seed=70)
    _, base = PR.accumulate(**s)
    live = np.nonzero(base > 0)[0]
    assert len(live) >= 12
    nan, inf = F("nan"), F("inf")
    for k, (col, x) in enumerate(((0, nan), (1, nan), (2, nan), (0, inf), (1, -inf), (2, inf))):
        s["points"][live[k], col] = x
        s["dirs"][live[6 + k], col] = x
    acc0 = dev(np.random.RandomState(1).rand(130, 4).astype(F))
    views0 = torch.arange(130, dtype=torch.int32, device="cuda")
    want_acc, want_views = PR.accumulate(**s, acc=acc0.cpu().numpy(), views=views0.cpu().numpy())
    acc, views = lib_accumulate(s, acc0.clone(), views0.clone())
    assert np.array_equal(bits(acc), PR.words(want_acc)) and np.array_equal(views.cpu().numpy(), want_views)
    bad, good = torch.from_numpy(live[:12]).cuda(), torch.from_numpy(live[12:]).cuda()
    assert torch.equal(acc[bad], acc0[bad]) and torch.equal(views[bad], views0[bad])
    assert (views[good] > views0[good]).all()
    rgb, seen = lib_resolve(acc, views, s["valid"])
    want_rgb, want_seen = PR.resolve(want_acc, want_views, s["valid"], 1)
    assert np.array_equal(bits(rgb), PR.words(want_rgb)) and np.array_equal(seen.cpu().numpy(), want_seen)


def test_bad_poses_read_nothing():
    """A pose of NaN fails test 1 and a pose at 1e30 fails test 3 for every point, so neither forms an index; the result is that of
    the other cameras alone."""
    s = PR.random_scene(257, (16, 12), 5, seed=80)
    s["poses"][1] = np.nan
    s["poses"][3, :, 3] = 1e30
    s["poses"][4, 0, 0] = np.inf
    acc, views = lib_accumulate(s)
    keep = [0, 2]
    want_acc, want_views = PR.accumulate(**{**s, "poses": s["poses"][keep], "images": s["images"][keep], "zbuf": s["zbuf"][keep]})
    assert want_views.sum() > 0
    assert np.array_equal(bits(acc), PR.words(want_acc)) and np.array_equal(views.cpu().numpy(), want_views)
    check(s)


# ---- 5. chunks of cameras and of points


def test_camera_chunks_with_carried_sums_equal_one_call():
    n_cams = TILE + 6
    s = PR.random_scene(257, (5, 7), n_cams, seed=90)
    whole_acc, whole_views = check(s)
    for cut in (1, TILE - 1, TILE, TILE + 1):
        acc, views = lib_accumulate(s, cams=slice(0, cut))
        acc, views = lib_accumulate(s, acc, views, cams=slice(cut, None))
        assert np.array_equal(bits(acc), PR.words(whole_acc)) and np.array_equal(views.cpu().numpy(), whole_views), cut
    acc = views = None
    for c0 in range(0, n_cams, 9):                      # many small chunks
        acc, views = lib_accumulate(s, acc, views, cams=slice(c0, c0 + 9))
    assert np.array_equal(bits(acc), PR.words(whole_acc)) and np.array_equal(views.cpu().numpy(), whole_views)


@pytest.mark.parametrize("chunk", [63, 257])
def test_point_chunks_equal_one_call(chunk):
    n = 600
    s = PR.random_scene(n, (16, 12), 3, seed=95)
    whole_acc, whole_views = check(s)
    acc, views = torch.zeros(n, 4, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    for p0 in range(0, n, chunk):                       # views into the one pair of buffers: row p0 of acc is 16-byte aligned
        lib_accumulate(s, acc[p0:p0 + chunk], views[p0:p0 + chunk], pts=slice(p0, p0 + chunk))
    assert np.array_equal(bits(acc), PR.words(whole_acc)) and np.array_equal(views.cpu().numpy(), whole_views)


# ---- 6. photo_colors: the depth buffers come from ngp_meshcull_views


def same_triple(got, want):
    """(rgb, seen, views) of the library and of the restatement, every bit."""
    return (np.array_equal(bits(got[0]), PR.words(want[0])) and np.array_equal(got[1].cpu().numpy(), want[1])
            and np.array_equal(got[2].cpu().numpy(), want[2]))


@pytest.fixture(scope="module")
def two_squares():
    K, poses, images, zbuf, face = PR.two_squares_scene()
    return dict(K=K, poses=poses, images=images, zbuf=zbuf, img_wh=(images.shape[2], images.shape[1]))


def test_photo_colors_chunked_by_workspace(two_squares):
    from ngp_pl_amd import mesh
    sc = two_squares
    W, H = sc["img_wh"]
    m = to_mesh(PR.TWO_V, PR.TWO_F, PR.TWO_N)
    g = np.random.RandomState(3)
    n = 700
    points = np.stack([g.uniform(-1.1, 1.1, n), g.uniform(-1.1, 1.1, n), g.choice([0.0, PR.GAP], n) + g.normal(0, 0.03, n)], 1).astype(F)
    dirs = np.tile(F([[0, 0, -1]]), (n, 1))
    valid = (g.rand(n) < 0.9).astype(np.uint8)
    args = (dev(points), dev(dirs), dev(valid), sc["images"], sc["K"], sc["poses"], sc["img_wh"])
    kw = dict(bias=PR.TWO_BIAS, guard=1, min_cos=0.1, power=2, near=0.01)
    # the cull's depth buffers are the reference raster's, bit for bit: photo_colors really used them
    views_v, zb = mesh.vertex_views(m, sc["K"], sc["poses"], sc["img_wh"], bias=PR.TWO_BIAS, near=0.01, return_zbuffer=True)
    assert np.array_equal(zb.cpu().numpy().view(np.uint32), sc["zbuf"])
    want = PR.photo_colors(PR.TWO_V, PR.TWO_F, points, dirs, valid, sc["images"], sc["K"], sc["poses"], sc["img_wh"], **kw)
    assert 100 < want[1].sum() < n and want[2].max() == 3
    whole = mesh.photo_colors(m, *args, **kw)
    assert same_triple(whole, want) and (whole[0].dtype, whole[1].dtype, whole[2].dtype) == (torch.float32, torch.uint8, torch.int32)
    for ws in (1, 7 * W * H, 7 * W * H * 2 + 5):         # one camera at a time (twice), two and one
        assert same_triple(mesh.photo_colors(m, *args, max_workspace_bytes=ws, **kw), want), ws
    # photographs already on the device, and min_views
    got = mesh.photo_colors(m, args[0], args[1], args[2], dev(sc["images"]), *args[4:], min_views=2, **kw)
    want2 = PR.photo_colors(PR.TWO_V, PR.TWO_F, points, dirs, valid, sc["images"], sc["K"], sc["poses"], sc["img_wh"], min_views=2, **kw)
    assert same_triple(got, want2) and want2[1].sum() < want[1].sum()
    # vertices are points like any other
    vn = mesh.photo_colors(m, m.vertices, -m.normals, torch.ones(8, dtype=torch.uint8, device="cuda"), *args[3:], **kw)
    assert vn[0].shape == (8, 3) and vn[1].shape == (8,) and vn[2].dtype == torch.int32


# ---- 7. bake_texture_from_images on the two squares


def _reference_bake(points, dirs, valid, sc, fill, **kw):
    rgb, seen, _ = PR.photo_colors(None, None, points, dirs, valid, sc["images"], sc["K"], sc["poses"], sc["img_wh"], zbuf=sc["zbuf"], near=0.01, **kw)
    colour = np.where(seen[:, None] == 1, rgb, F(fill)[None])
    image = PR.quantise(colour)
    image[valid == 0] = 0
    return image, seen


@pytest.mark.parametrize("kind", ["uniform", "adaptive"])
def test_bake_texture_from_images(two_squares, kind):
    from ngp_pl_amd import mesh
    sc = two_squares
    m = to_mesh(PR.TWO_V, PR.TWO_F, PR.TWO_N)
    cam = dict(images=sc["images"], K=sc["K"], poses=sc["poses"], img_wh=sc["img_wh"])
    kw = dict(bias=PR.TWO_BIAS, guard=1, min_cos=0.1, power=2)
    if kind == "uniform":
        atlas = dict(texels=PR.TWO_TEXELS)
        p, d, valid = TR.texel_points(PR.TWO_V, PR.TWO_F, PR.TWO_N, PR.TWO_TEXELS, PR.TWO_BOX)
        owner = TR.owners(len(PR.TWO_F), PR.TWO_TEXELS)[0]
    else:
        atlas = dict(texel_size=0.1)                     # the rear faces get 32 texels a leg, the front ones 16
        a = AR.Atlas(PR.TWO_V, PR.TWO_F, F(0.1))
        assert sorted(set(a.face_texels.tolist())) == [16, 32]
        p, d, valid = AR.texel_points(PR.TWO_V, PR.TWO_F, PR.TWO_N, a.order, a.counts, PR.TWO_BOX)
        owner = AR.owners(a.order, a.counts)[0]
    magenta = (1, 0, 1)
    want, want_seen = _reference_bake(p, d, valid, sc, magenta, **kw)
    got, seen = mesh.bake_texture_from_images(m, **cam, **atlas, **kw, fill=magenta, box=PR.TWO_BOX, return_seen=True)
    t = got.texture
    assert isinstance(t, mesh.Texture if kind == "uniform" else mesh.AdaptiveTexture) and t.image.dtype == torch.uint8
    assert seen.dtype == torch.uint8 and tuple(seen.shape) == (t.height, t.width) and tuple(t.image.shape) == (t.height, t.width, 3)
    image = t.image.cpu().numpy().reshape(-1, 3)
    assert np.array_equal(seen.cpu().numpy().reshape(-1), want_seen) and np.array_equal(image, want)
    # unseen valid texels are magenta, invalid ones 0, and the squares keep their colours (tests/test_meshphoto_cpu.py)
    ok, sn = valid == 1, want_seen == 1
    assert (ok & ~sn).sum() > 50 and (image[ok & ~sn] == (255, 0, 255)).all() and not image[~ok].any()
    assert (image[sn & (owner < 2)] == PR.REAR_RGB).all() and (image[sn & (owner >= 2)] == PR.FRONT_RGB).all() and sn.sum() > 600
    # the atlas is bake_texture's, and baking twice, in other chunks, gives the same bytes
    again = mesh.bake_texture_from_images(m, **cam, **atlas, **kw, fill=magenta, box=PR.TWO_BOX, chunk=257).texture
    assert torch.equal(again.image, t.image) and (again.width, again.height) == (t.width, t.height)
    blank = mesh.texture_atlas(m, **atlas)
    assert (blank.width, blank.height) == (t.width, t.height) and torch.equal(blank.uvs, t.uvs)
    # default fill: black; with a model: the field's colour where no photograph sees, as bake_texture evaluates it

    class Flat(torch.nn.Module):
        xyz_min, xyz_max = torch.tensor([-2.0, -2.0, -2.0]), torch.tensor([2.0, 2.0, 2.0])

        def forward(self, p, d):
            return None, torch.stack([0.25 + 0.0 * p[:, 0], 0.5 + 0.1 * p[:, 1], 0.75 + 0.0 * p[:, 2]], 1)

    black = mesh.bake_texture_from_images(m, **cam, **atlas, **kw, box=PR.TWO_BOX).texture.image.cpu().numpy().reshape(-1, 3)
    assert not black[~sn].any() and np.array_equal(black[sn], want[sn])
    field = mesh.bake_texture(Flat(), m, **atlas).texture.image.cpu().numpy().reshape(-1, 3)
    mixed = mesh.bake_texture_from_images(m, **cam, **atlas, **kw, model=Flat()).texture.image.cpu().numpy().reshape(-1, 3)
    assert np.array_equal(mixed[sn], want[sn]) and np.array_equal(mixed[~sn], field[~sn]) and field[ok & ~sn].any()


# ---- 8. extract_mesh and the CLI on a small model


def test_extract_mesh_and_the_cli(true_density, tmp_path, capsys):
    from ngp_pl_amd import mesh, synthetic as syn
    from tests.test_meshtex_cpu import read_png
    model = make_model()
    res = 32
    kw = dict(keep_largest=1)
    plain = mesh.extract_mesh(model, res, **kw)
    # no existing behaviour changes: without images the texture is bake_texture's, as before
    today = mesh.extract_mesh(model, res, texture=2, **kw)
    field = mesh.bake_texture(model, plain, 2).texture
    assert same_mesh(today, plain) and torch.equal(today.texture.image, field.image) and torch.equal(today.texture.uvs, field.uvs)
    W = H = 48
    K, poses = syn.intrinsics(W), syn.hemisphere_poses(4, seed=1)
    photos = np.random.RandomState(0).randint(0, 256, (4, H, W, 3)).astype(np.uint8)
    cam = dict(images=photos, K=K, poses=poses, img_wh=(W, H))
    lo, hi = mesh._bounds(model, None)
    bias = 2.0 * max((b - a) / (res - 1) for a, b in zip(lo, hi))
    p, d, ok = mesh.texel_points(plain, field, mesh._box(model))
    rgb, seen, _ = mesh.photo_colors(plain, p, d, ok, photos, K, poses, (W, H), bias=bias)
    share = seen.sum().item() / ok.sum().item()
    assert 0.05 < share < 1
    want = torch.where(seen.bool().unsqueeze(1), mesh._quantise(rgb), field.image.view(-1, 3))
    for texture in (dict(texels=2, images=cam), dict(texels=2, images=dict(cam, bias=bias, guard=1, min_cos=0.1, power=2, min_views=1))):
        got = mesh.extract_mesh(model, res, texture=texture, **kw)
        assert same_mesh(got, plain) and isinstance(got.texture, mesh.Texture) and torch.equal(got.texture.uvs, field.uvs)
        assert torch.equal(got.texture.image.view(-1, 3), want) and not torch.equal(got.texture.image, field.image)
    # with smoothing the bake still happens before it, on the geometry the photographs saw
    smooth = mesh.extract_mesh(model, res, smooth=2, texture=dict(texels=2, images=cam), **kw)
    assert torch.equal(smooth.texture.image.view(-1, 3), want) and not torch.equal(smooth.vertices, plain.vertices)
    # the adaptive atlas takes the same option
    adaptive = mesh.extract_mesh(model, res, texture=dict(texel_size=0.5, images=dict(cam, min_views=2)), **kw)
    direct = mesh.bake_texture_from_images(plain, **cam, texel_size=0.5 * bias / 2.0, bias=bias, min_views=2, model=model)
    assert isinstance(adaptive.texture, mesh.AdaptiveTexture) and torch.equal(adaptive.texture.image, direct.texture.image)
    # the CLI
    slim = {"model." + k: x.detach().cpu() for k, x in model.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt, out, npz = str(tmp_path / "slim.ckpt"), str(tmp_path / "scene.obj"), str(tmp_path / "photos.npz")
    torch.save(slim, ckpt)
    np.savez(npz, K=K.numpy(), poses=np.asarray(poses), img_wh=np.array([W, H]), images=photos)
    capsys.readouterr()
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--keep-largest", "1", "--texture-texels", "2", "--texture-images", npz, "--out", out]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    record = json.loads(lines[-1])["texture_images"]
    assert record == dict(cameras=4, valid_texels=int(ok.sum().item()), seen_texels=int(seen.sum().item()), seen_share=share)
    assert sorted(os.listdir(str(tmp_path))) == ["photos.npz", "scene.mtl", "scene.obj", "scene.png", "slim.ckpt"]
    assert np.array_equal(read_png(str(tmp_path / "scene.png")), want.view(field.height, field.width, 3).cpu().numpy())
    # the options reach the bake: a stricter angle and two views see less
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--keep-largest", "1", "--texture-texels", "2", "--texture-images", npz,
                      "--texture-image-bias", repr(bias), "--texture-image-guard", "2", "--texture-image-min-cos", "0.5", "--texture-image-power", "4",
                      "--texture-image-min-views", "2", "--out", out]) == 0
    strict = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["texture_images"]
    _, seen2, _ = mesh.photo_colors(plain, p, d, ok, photos, K, poses, (W, H), bias=bias, guard=2, min_cos=0.5, power=4, min_views=2)
    assert strict["seen_texels"] == int(seen2.sum().item()) < record["seen_texels"] and strict["valid_texels"] == record["valid_texels"]
