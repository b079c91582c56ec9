"""GPU: the depth-map fusion of libngp_meshtsdf.so, bit for bit against the numpy restatement (tests/mesh_tsdf_reference.py): state
and volume on a lattice whose rows and waves do not align, cameras inside the box and looking away, depth maps with patches of
+inf, NaN, 0 and negatives, camera chunking across more than one LDS tile, determinism, the analytic sphere scene through marching
cubes and the component labelling, render_depths on a trained field, and the model path (extract_mesh(tsdf=...), the CLI).  Nothing
here has a tolerance except where marching cubes is compared as tests/test_mesh_gpu.py compares it."""
import numpy as np
import pytest
import torch

from ngp_pl_amd import synthetic as syn
from tests import mc_reference as R
from tests import mesh_tsdf_reference as TR
from tests import mesh_visibility_reference as VR

pytestmark = pytest.mark.gpu

BOX = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def gpu_tsdf(resolution, bounds, K, poses, wh, depths, near, trunc, **kw):
    """acc, seen, behind (n,) and vol (nz, ny, nx) of the GPU as numpy."""
    from ngp_pl_amd import mesh
    nx, ny, nz = resolution
    vol, acc, seen, behind = mesh.tsdf_volume(resolution, bounds, torch.from_numpy(K), torch.from_numpy(poses), wh, torch.from_numpy(depths).cuda(),
                                              trunc, near=near, return_state=True, **kw)
    assert vol.shape == acc.shape == seen.shape == behind.shape == (nz, ny, nx)
    assert vol.dtype == acc.dtype == torch.float32 and seen.dtype == behind.dtype == torch.int32
    return acc.cpu().numpy().reshape(-1), seen.cpu().numpy().reshape(-1), behind.cpu().numpy().reshape(-1), vol.cpu().numpy()


def assert_same(got, want):
    for name, g, w in zip(("acc", "seen", "behind", "vol"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        assert np.array_equal(bits(g), bits(w)), "%s: %d of %d words differ" % (name, (bits(g) != bits(w)).sum(), g.size)


def patched(depths):
    """Patches of +inf, NaN, 0 and a negative value in every depth map, over pixels the lattice projects to."""
    d = depths.copy()
    H, W = d.shape[1:]
    d[:, H // 4:H // 4 + 5, W // 3:W // 3 + 7] = np.inf
    d[:, H // 2:H // 2 + 6, W // 2 - 3:W // 2 + 4] = np.nan
    d[:, H // 2 - 9:H // 2 - 4, W // 4:W // 4 + 6] = 0.0
    d[:, 2 * H // 3:2 * H // 3 + 4, W // 2:W // 2 + 9] = -1.25
    return d


@pytest.mark.parametrize("K,wh", [(VR.intrinsics(70, 32, 32), (64, 64)), (VR.intrinsics(61, 20.25, 55.5), (53, 97))],
                         ids=["square", "non_square_offset_principal_point"])
def test_state_and_volume_exact(K, wh):
    """24 x 20 x 17 points: a wave of 64 spans 2.7 rows.  Three cameras of the hemisphere kind, one close to the box, one inside the
    box looking away from the sphere (part of the lattice is behind it, part beside it)."""
    res, bounds = (24, 20, 17), ((-0.5, -0.45, -0.4), (0.5, 0.4, 0.45))
    poses = np.concatenate([syn.hemisphere_poses(3, seed=4).numpy(),
                            np.stack([VR.look_at((0.7, -0.6, 0.2), (0, 0, 0)), VR.look_at((0.1, 0.05, 0.0), (0.45, 0.4, 0.3))])]).astype(np.float32)
    depths = patched(TR.sphere_depths(K, poses, wh, 0.3))
    near, trunc = 0.05, 4.0 / 23
    want = TR.tsdf(res, bounds, K, poses, wh, depths, near, trunc)
    acc, seen, behind, vol = want
    # the scene exercises every branch of the rule
    assert (seen == 0).sum() > 50 and (behind > 0).sum() > 200 and ((seen == 0) & (behind > 0)).sum() > 20
    assert ((seen > 0) & (behind > 0)).sum() > 200 and (seen == 5).sum() > 0 and 0 < (seen + behind < 5).sum()
    assert (np.abs(vol) < 1).sum() > 500 and (vol == 1).sum() > 20 and (vol == -1).sum() > 500
    for special in (np.isnan(depths), depths == 0, depths < 0, np.isinf(depths)):
        assert special.all(0).any()
    inside = TR.integrate(TR.lattice(res, bounds), K, poses[4:], wh, depths[4:], near, trunc, TR.clear(24 * 20 * 17))
    assert 0 < (inside[1] + inside[2] > 0).sum() < 24 * 20 * 17 // 2             # the camera inside sees less than half the lattice
    got = gpu_tsdf(res, bounds, K, poses, wh, depths, near, trunc)
    assert_same(got, want)
    from ngp_pl_amd import mesh
    alone = mesh.tsdf_volume(res, bounds, K, poses, wh, torch.from_numpy(depths).cuda(), trunc, near=near)      # vol written over acc
    assert np.array_equal(bits(alone), bits(vol))


def test_camera_chunks_give_identical_state():
    """130 cameras: two LDS tiles of 128 in one call; one camera per call; chunks of 7 (18 of 7 and one of 4)."""
    res, wh, near, trunc = (9, 9, 9), (16, 12), 0.05, 0.25
    K = VR.intrinsics(14, 8, 6)
    poses = syn.hemisphere_poses(130, seed=7).numpy()
    depths = TR.sphere_depths(K, poses, wh, 0.3)
    depths[::3, 5:8, 6:10] = np.nan
    want = TR.tsdf(res, BOX, K, poses, wh, depths, near, trunc)
    assert want[1].max() > 100 and want[2].max() > 20 and len(np.unique(want[0])) > 200
    assert_same(gpu_tsdf(res, BOX, K, poses, wh, depths, near, trunc), want)
    assert_same(gpu_tsdf(res, BOX, K, poses, wh, depths, near, trunc, max_cameras_per_call=1), want)
    assert_same(gpu_tsdf(res, BOX, K, poses, wh, depths, near, trunc, max_cameras_per_call=7), want)
    # the sum is sequential in camera order: the other order gives other bits somewhere, the same counts everywhere
    back = TR.tsdf(res, BOX, K, poses[::-1], wh, depths[::-1], near, trunc)
    assert np.array_equal(back[1], want[1]) and np.array_equal(back[2], want[2]) and not np.array_equal(bits(back[0]), bits(want[0]))
    assert_same(gpu_tsdf(res, BOX, K, poses[::-1].copy(), wh, depths[::-1].copy(), near, trunc, max_cameras_per_call=50), back)


@pytest.fixture(scope="module")
def sphere():
    """The sphere scene of tests/test_meshtsdf_cpu.py and the restatement's state and volume on it (computed once)."""
    K, poses, depths = TR.sphere_scene()
    S = TR.SPHERE
    return K, poses, depths, TR.tsdf(S["resolution"], S["bounds"], K, poses, S["img_wh"], depths, S["near"], S["trunc"])


def sphere_volume(sphere, **kw):
    from ngp_pl_amd import mesh
    K, poses, depths, _ = sphere
    S = TR.SPHERE
    return mesh.tsdf_volume(S["resolution"], S["bounds"], K, poses, S["img_wh"], torch.from_numpy(depths).cuda(), S["trunc"], near=S["near"], **kw)


def test_two_runs_are_bit_identical(sphere):
    a, b = sphere_volume(sphere, return_state=True), sphere_volume(sphere, return_state=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_sphere_scene_volume_mesh_and_components(sphere):
    from ngp_pl_amd import mesh
    K, poses, depths, want = sphere
    S = TR.SPHERE
    assert_same(gpu_tsdf(S["resolution"], S["bounds"], K, poses, S["img_wh"], depths, S["near"], S["trunc"]), want)
    vol = sphere_volume(sphere)
    m = mesh.marching_cubes(vol, 0.0, S["bounds"])
    rv, rf, rn, _ = R.marching_cubes(vol.cpu().numpy(), 0.0, *S["bounds"])
    v, f, n = m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.normals.cpu().numpy()
    assert len(rf) == 7580 and f.dtype == np.int32 and np.array_equal(f, rf)
    assert v.shape == rv.shape and np.abs(v - rv).max() <= 1e-6 * 1.0
    assert np.abs(n - rn).max() <= 1e-5
    assert mesh.connected_components(m).n_components == 1
    assert R.is_closed_oriented(f) and R.euler(v, f) == 2


def make_model(seed=3):
    from ngp_pl_amd.networks import NGP
    torch.manual_seed(seed)
    m = NGP(scale=0.5).cuda()
    m.register_training_buffers()
    return m


def ray_batch(n, seed, W=200):
    g = np.random.RandomState(seed)
    K = syn.intrinsics(W)
    dirs = syn.get_ray_directions(W, W, K)
    poses = syn.hemisphere_poses(16, seed=1)
    img = torch.from_numpy(g.randint(0, 16, n))
    pix = torch.from_numpy(g.randint(0, W * W, n))
    ro, rd = syn.get_rays(dirs[pix], poses[img])
    ro, rd = ro.cuda(), rd.cuda()
    gt, _ = syn.render_ground_truth(ro, rd, n_steps=192)
    return ro.contiguous(), rd.contiguous(), gt.contiguous()


@pytest.fixture(scope="module")
def trained():
    """The short training of tests/test_mesh_gpu.py: 2 000 native steps of 4096 rays on the procedural scene."""
    from ngp_pl_amd.trainer import Trainer
    model = make_model(seed=2)
    tr = Trainer(model)
    batches = [ray_batch(4096, seed=500 + i) for i in range(16)]
    for it in range(2000):
        ro, rd, gt = batches[it % 16]
        nxt = batches[(it + 1) % 16]
        tr.step(ro, rd, gt, next_batch=(nxt[0], nxt[1]))
    torch.cuda.synchronize()
    return model


def test_render_depths_is_the_renderers_depth_over_opacity(trained):
    from ngp_pl_amd import mesh
    from ngp_pl_amd.rendering import render
    W, H = 64, 48
    K, poses = syn.intrinsics(W, H), syn.hemisphere_poses(2, seed=1)
    got = mesh.render_depths(trained, K, poses, (W, H))
    assert got.shape == (2, H, W) and got.dtype == torch.float32 and got.is_cuda
    dirs = syn.get_ray_directions(H, W, K, device="cuda")
    for c in range(2):
        ro, rd = syn.get_rays(dirs, poses[c].cuda())
        r = render(trained, ro, rd, test_time=True)
        opaque = r["opacity"] >= 0.5
        assert opaque.sum() > 100 and (~opaque).sum() > 100                     # both classes: the object and the empty frame around it
        want = torch.where(opaque, r["depth"] / r["opacity"], torch.full_like(r["depth"], float("inf"))).view(H, W)
        assert torch.equal(got[c].view(torch.int32), want.view(torch.int32))
        assert (got[c][opaque.view(H, W)] > 0.5).all() and (got[c][opaque.view(H, W)] < 2.5).all()      # cameras at 1.5 from a unit box
        assert torch.isinf(got[c][~opaque.view(H, W)]).all()
    again = mesh.render_depths(trained, K, poses, (W, H))
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    # a higher bar leaves fewer surface pixels
    strict = mesh.render_depths(trained, K, poses, (W, H), min_opacity=0.999)
    assert torch.isfinite(strict).sum() < torch.isfinite(got).sum() and torch.equal(strict[torch.isfinite(strict)], got[torch.isfinite(strict)])


@pytest.fixture
def true_density(monkeypatch):
    """The model's density lattice replaced by the procedural scene's true density, as tests/test_mesh_gpu.py samples it."""
    from ngp_pl_amd import mesh

    def volume(model, resolution=512, bounds=None, chunk=0):
        nx, ny, nz = mesh._resolution(resolution)
        xyz = mesh.lattice_points((nx, ny, nz), mesh._bounds(model, bounds))
        return syn.density(xyz).view(nz, ny, nx).contiguous()

    monkeypatch.setattr(mesh, "density_volume", volume)


def same_mesh(a, b):
    ok = torch.equal(a.faces, b.faces) and torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))
    return ok and torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32))


def test_extract_mesh_with_tsdf_from_given_depths(sphere, true_density):
    from ngp_pl_amd import mesh
    K, poses, depths, _ = sphere
    S = TR.SPHERE
    model = make_model()
    res, wh = 48, S["img_wh"]
    d = torch.from_numpy(depths).cuda()
    opts = dict(K=K, poses=poses, img_wh=wh, depths=d)
    got = mesh.extract_mesh(model, res, tsdf=opts)
    lo, hi = mesh._box(model)
    assert (tuple(lo), tuple(hi)) == S["bounds"]
    want = mesh.marching_cubes(mesh.tsdf_volume(res, (lo, hi), K, poses, wh, d, 4.0 * (1.0 / 47)), 0.0, (lo, hi))
    assert got.faces.shape == (7580, 3) and same_mesh(got, want) and got.colors is None
    assert same_mesh(mesh.extract_mesh(model, res, threshold=-123.0, tsdf=opts), want)          # the threshold is not used
    wide = mesh.extract_mesh(model, res, tsdf=dict(opts, trunc_voxels=6.0))
    assert same_mesh(wide, mesh.marching_cubes(mesh.tsdf_volume(res, (lo, hi), K, poses, wh, d, 6.0 * (1.0 / 47)), 0.0, (lo, hi)))
    assert not torch.equal(wide.vertices, want.vertices)
    # the later stages follow in their order: filter, cull, simplify
    cull = dict(K=K, poses=poses, img_wh=wh)
    staged = mesh.extract_mesh(model, res, tsdf=opts, keep_largest=1, cull=cull, simplify_voxels=2)
    by_hand = mesh.filter_components(want, keep_largest=1)
    by_hand = mesh.cull_invisible(by_hand, K, poses, wh, 2.0 * (1.0 / 47))
    by_hand = mesh.simplify_clusters(by_hand, 2.0 * (1.0 / 47), origin=lo)
    assert 0 < staged.faces.shape[0] < want.faces.shape[0] and same_mesh(staged, by_hand)
    # tsdf=None: the density path of before
    plain = mesh.extract_mesh(model, 64, 20.0)
    assert same_mesh(mesh.extract_mesh(model, 64, 20.0, tsdf=None), plain)
    assert same_mesh(plain, mesh.marching_cubes(mesh.density_volume(model, 64, (lo, hi)), 20.0, (lo, hi))) and plain.faces.shape[0] > 1000


def test_cli_tsdf_cameras(trained, tmp_path, capsys):
    from ngp_pl_amd import mesh
    from ngp_pl_amd.networks import NGP
    from ngp_pl_amd.utils import load_ckpt
    from tests.test_meshfilter_gpu import read_ply
    res, W = 48, 48
    K, poses = syn.intrinsics(W), syn.hemisphere_poses(6, seed=2)
    slim = {"model." + k: v.detach().cpu() for k, v in trained.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt, out, cams = str(tmp_path / "slim.ckpt"), str(tmp_path / "m.ply"), str(tmp_path / "cams.npz")
    torch.save(slim, ckpt)
    np.savez(cams, K=K.numpy(), poses=poses.numpy(), img_wh=np.array([W, W]))
    model = NGP(scale=0.5).cuda()                        # as the CLI loads it
    load_ckpt(model, ckpt, prefixes_to_ignore=("density_grid", "grid_coords"))
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--tsdf-cameras", cams, "--out", out]) == 0
    want = mesh.extract_mesh(model, res, tsdf=dict(K=K, poses=poses, img_wh=(W, W)))
    verts, faces = read_ply(out)
    assert want.faces.shape[0] > 100
    assert np.array_equal(faces, want.faces.cpu().numpy()) and np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), want.vertices.cpu().numpy())
    last = capsys.readouterr().out.strip().splitlines()[-1]
    assert last == "%s: %d vertices, %d faces, tsdf from 6 cameras" % (out, len(verts), len(faces))
    # the options, with the component filter behind
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--tsdf-cameras", cams, "--tsdf-trunc-voxels", "3", "--tsdf-min-opacity", "0.8",
                      "--keep-largest", "1", "--out", out]) == 0
    want = mesh.extract_mesh(model, res, tsdf=dict(K=K, poses=poses, img_wh=(W, W), trunc_voxels=3.0, min_opacity=0.8), keep_largest=1)
    verts, faces = read_ply(out)
    assert len(faces) > 0 and np.array_equal(faces, want.faces.cpu().numpy())
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), want.vertices.cpu().numpy())
    import re
    last = capsys.readouterr().out.strip().splitlines()[-1]
    assert re.fullmatch(re.escape("%s: %d vertices, %d faces, tsdf from 6 cameras, " % (out, len(verts), len(faces))) + r"\d+ components found, 1 kept", last)
    # without the option: the line of before
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--out", out]) == 0
    verts, faces = read_ply(out)
    assert capsys.readouterr().out.strip().splitlines()[-1] == "%s: %d vertices, %d faces" % (out, len(verts), len(faces))
