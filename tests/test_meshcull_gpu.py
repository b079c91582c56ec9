"""GPU: the depth-buffer visibility test and the cull of libngp_meshcull.so, bit for bit against the numpy restatement
(tests/mesh_visibility_reference.py): depth buffers, vertex_views and the culled mesh on the two-shell scene, camera chunking, a
non-square image with cameras inside the mesh and looking away, the wave-walked large boxes, the edge rules, determinism, and
the model path (extract_mesh(cull=...), the CLI).  About 0.1 % of the (vertex, camera) pairs of the scene lie within 1e-3 * bias
of the threshold: a count that differs is an arithmetic-order bug, which is why nothing here has a tolerance."""
import numpy as np
import pytest
import torch

from tests import mc_reference as R
from tests import mesh_visibility_reference as VR

pytestmark = pytest.mark.gpu

WH, NEAR, BIAS = (96, 64), 0.05, 2 / 39


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def to_mesh(v, f, n=None, c=None, device="cuda"):
    from ngp_pl_amd import mesh
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return mesh.Mesh(t(v), t(f), t(n), t(c))


def gpu_views(v, f, K, poses, wh, bias, near, **kw):
    """vertex_views and the depth workspace of the GPU, as numpy i32 / u32."""
    from ngp_pl_amd import mesh
    views, zb = mesh.vertex_views(to_mesh(v, f), torch.from_numpy(K), torch.from_numpy(poses), wh, bias, near=near, return_zbuffer=True, **kw)
    assert views.dtype == torch.int32 and views.shape == (len(v),)
    return views.cpu().numpy(), zb.cpu().numpy().view(np.uint32)


def check_exact(v, f, K, poses, wh, bias, near):
    """One chunk: depth buffers and views against the restatement; returns the restatement's."""
    want_zb = VR.zbuffers(v, f, K, poses, wh, near)
    want = VR.vertex_views(v, f, K, poses, wh, bias, near, want_zb)
    got, got_zb = gpu_views(v, f, K, poses, wh, bias, near)
    assert got_zb.shape == want_zb.shape
    assert np.array_equal(got_zb, want_zb), "%d depth words differ" % (got_zb != want_zb).sum()
    assert np.array_equal(got, want), "%d vertex counts differ" % (got != want).sum()
    return want, want_zb


def check_cull(m, v, f, n, c, views, K, poses, wh, bias, near, min_views):
    from ngp_pl_amd import mesh
    got = mesh.cull_invisible(m, torch.from_numpy(K), torch.from_numpy(poses), wh, bias, min_views=min_views, near=near)
    wv, wf, wn, wc = VR.cull(v, f, views, min_views, n, c)
    assert got.faces.dtype == torch.int32 and got.faces.shape == wf.shape and np.array_equal(got.faces.cpu().numpy(), wf)
    assert got.vertices.shape == wv.shape and np.array_equal(bits(got.vertices), bits(wv))
    for a, w in ((got.normals, wn), (got.colors, wc)):
        assert (a is None) == (w is None)
        if w is not None:
            assert a.shape == w.shape and np.array_equal(bits(a), bits(w))
    return got


@pytest.fixture(scope="module")
def scene():
    """The two-shell scene of tests/test_meshcull_cpu.py and the restatement's depth buffers and views on it (computed once)."""
    v, f, n, _ = R.marching_cubes(VR.shells_volume(), 0.0, (0, 0, 0), (1, 1, 1))
    K, poses = VR.intrinsics(70, 48, 32), VR.ring_cameras()
    zb = VR.zbuffers(v, f, K, poses, WH, NEAR)
    views = VR.vertex_views(v, f, K, poses, WH, BIAS, NEAR, zb)
    assert v.shape == (8688, 3) and f.shape == (17360, 3) and (views > 0).sum() == 4632
    return v, f, n, K, poses, zb, views


def test_scene_depth_buffers_and_views_exact(scene):
    v, f, n, K, poses, want_zb, want = scene
    got, got_zb = gpu_views(v, f, K, poses, WH, BIAS, NEAR)
    assert got_zb.shape == (14, 64, 96)
    assert np.array_equal(got_zb, want_zb), "%d depth words differ" % (got_zb != want_zb).sum()
    assert np.array_equal(got, want), "%d vertex counts differ" % (got != want).sum()


@pytest.mark.parametrize("min_views", [1, 4, 8])
def test_scene_culled_mesh_exact_with_attributes_riding_along(scene, min_views):
    from ngp_pl_amd import mesh
    v, f, n, K, poses, _, views = scene
    g = np.random.RandomState(min_views)
    # any bit pattern must survive the copy (NaN payloads, denormals, -0)
    nrm, col = [g.randint(-2 ** 31, 2 ** 31, v.shape, dtype=np.int64).astype(np.int32).view(np.float32) for _ in range(2)]
    got = check_cull(to_mesh(v, f, nrm, col), v, f, nrm, col, views, K, poses, WH, BIAS, NEAR, min_views)
    if min_views == 8:
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and got.normals.shape == (0, 3) and got.colors.shape == (0, 3)
    else:                                                # the outer sheet, whole
        fo = got.faces.cpu().numpy()
        assert got.vertices.shape == (4632, 3) and R.is_closed_oriented(fo) and R.euler(got.vertices.cpu().numpy(), fo) == 2
    bare = check_cull(to_mesh(v, f), v, f, None, None, views, K, poses, WH, BIAS, NEAR, min_views)
    assert bare.normals is None and bare.colors is None
    m = to_mesh(v, f)
    assert mesh.cull_invisible(m, K, poses, WH, BIAS, min_views=0) is m


def test_camera_chunks_give_identical_views(scene):
    v, f, n, K, poses, want_zb, want = scene
    per_cam = 4 * WH[0] * WH[1]
    got, zb = gpu_views(v, f, K, poses, WH, BIAS, NEAR, max_zbuffer_bytes=3 * per_cam + 100)        # 3 + 3 + 3 + 3 + 2
    assert zb.shape == (3, 64, 96) and np.array_equal(got, want)
    assert np.array_equal(zb[:2], want_zb[12:])          # the workspace holds the last chunk
    got1, zb1 = gpu_views(v, f, K, poses, WH, BIAS, NEAR, max_zbuffer_bytes=1)                      # at least one camera
    assert zb1.shape == (1, 64, 96) and np.array_equal(got1, want) and np.array_equal(zb1[0], want_zb[13])


def test_non_square_offset_cameras_inside_and_looking_away():
    """(nz, ny, nx) = (72, 56, 40), W x H = 53 x 97, principal point off centre.  Camera 4 sits inside the outer shell's wall, so
    faces cross its near plane (they occlude nothing); camera 5 looks away from the mesh."""
    v, f, n, _ = R.marching_cubes(VR.shells_volume((72, 56, 40)), 0.0, (0, 0, 0), (1, 1, 1))
    K = VR.intrinsics(61, 20.25, 55.5)
    c = np.array([0.5, 0.5, 0.5])
    poses = np.stack([VR.look_at(c + 1.4 * np.array(d) / np.linalg.norm(d), c) for d in ((1, 0.2, 0.1), (-0.3, 1, 0.4), (0.2, -0.5, 1), (-1, -1, -0.7))]
                     + [VR.look_at(c + np.array([0.35, 0.0, 0.0]), c), VR.look_at(c + np.array([0.0, 1.5, 0.0]), c + np.array([0.0, 3.0, 0.0]))])
    wh, near, bias = (53, 97), 0.05, 2 / 39
    views, zb = check_exact(v, f, K, poses, wh, bias, near)
    u, vv, d = VR.project(v, K, poses[4])
    crossing = (d[f] >= near).any(1) & (d[f] < near).any(1)
    assert crossing.sum() > 10                                                 # faces across camera 4's near plane
    own = VR.vertex_views(v, f, K, poses[4:5], wh, bias, near)
    assert own.sum() > 10                                                      # it sees a little of the sheet in front of it
    assert (zb[5] == VR.INF_BITS).all() and VR.vertex_views(v, f, K, poses[5:6], wh, bias, near).sum() == 0
    assert views.max() >= 3 and (views == 0).sum() > 1000
    check_cull(to_mesh(v, f, n), v, f, n, None, views, K, poses, wh, bias, near, 1)
    check_cull(to_mesh(v, f, n), v, f, n, None, views, K, poses, wh, bias, near, 2)


def test_large_boxes_are_walked_by_the_wave(scene):
    """A two-triangle quad in front of camera 0 that fills its image (its corners project outside: the clipped box is the whole
    image, 6144 pixels), its faces in the middle of the 17 360 one-pixel faces."""
    v, f, n, K, poses, _, views = scene
    quad = np.array([[1.5, -0.2, -0.2], [1.5, 1.2, -0.2], [1.5, 1.2, 1.2], [1.5, -0.2, 1.2]], np.float32)      # camera 0 is at x = 2
    n_v = len(v)
    v2 = np.concatenate([v, quad])
    f2 = np.concatenate([f[:9000], np.array([[n_v, n_v + 1, n_v + 2], [n_v + 2, n_v + 3, n_v]], np.int32), f[9000:]])
    got, zb = check_exact(v2, f2, K, poses, WH, BIAS, NEAR)
    assert (zb[0].view(np.float32) == 0.5).all()                               # the quad, everywhere, in front of the shells
    # every shell vertex loses camera 0's view and keeps the others
    cam0 = VR.vertex_views(v, f, K, poses[:1], WH, BIAS, NEAR)
    assert cam0.sum() > 1000 and np.array_equal(got[:n_v], views - cam0)
    assert VR.vertex_views(v2, f2, K, poses[:1], WH, BIAS, NEAR)[:n_v].sum() == 0
    # a large face seen at a slant by several cameras: both windings, several large boxes in one wave
    tilted = np.array([[0.95, 0.0, 0.1], [1.0, 1.0, 0.0], [0.9, 0.9, 1.0], [1.0, 0.1, 0.95]], np.float32)
    v3 = np.concatenate([v, tilted])
    f3 = np.concatenate([np.array([[n_v, n_v + 1, n_v + 2], [n_v, n_v + 3, n_v + 2]], np.int32), f])
    check_exact(v3, f3, K, poses, WH, BIAS, NEAR)


def test_edge_rules():
    from ngp_pl_amd import mesh
    K = VR.intrinsics(10, 8, 8)
    pose = VR.look_at((0, 0, -2.0), (0, 0, 0), up=(0, -1, 0))[None]
    v = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [0.05, 0.05, 1], [4.0, 0, 3], [0, 0, -3]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 0, 1], [0, 1, 9], [-1, 1, 2], [2 ** 31 - 1, 0, 1]], np.int32)      # 3 of them out of range
    views, zb = check_exact(v, f, K, pose, (16, 16), 0.25, 0.05)
    assert views.tolist() == [1, 1, 1, 1, 0, 0, 0]        # occluded, exactly on the border u == W, behind the camera
    assert VR.project(v, K, pose[0])[0][5] == 16
    assert (zb[0] != VR.INF_BITS).sum() == 100
    got = check_cull(to_mesh(v, f), v, f, None, None, views, K, pose, (16, 16), 0.25, 0.05, 1)
    assert got.faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 0, 1]] and got.vertices.shape == (4, 3)     # the degenerate face rides on vertex 0
    check_exact(v, f, K, pose, (16, 16), 1.0, 0.05)
    check_exact(v, np.array([[0, 1, 6]], np.int32), K, pose, (16, 16), 0.25, 0.05)                      # across the near plane
    check_exact(v, f[:2, ::-1].copy(), K, pose, (16, 16), 0.25, 0.05)                                  # the other winding
    # zero faces: every vertex in front of the camera and inside the image is seen
    none, zb0 = check_exact(v, f[:0], K, pose, (16, 16), 0.25, 0.05)
    assert none.tolist() == [1, 1, 1, 1, 1, 0, 0] and (zb0 == VR.INF_BITS).all()
    e = mesh.cull_invisible(to_mesh(v, f[:0]), K, pose, (16, 16), 0.25)
    assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3)
    # zero vertices
    empty = to_mesh(v[:0], f[:0])
    assert mesh.vertex_views(empty, K, pose, (16, 16), 0.25).shape == (0,)
    e = mesh.cull_invisible(empty, K, pose, (16, 16), 0.25)
    assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3)
    # a 1 x 1 image
    check_exact(v, f, VR.intrinsics(10, 0.5, 0.5), pose, (1, 1), 0.25, 0.05)


def test_two_runs_are_bit_identical(scene):
    from ngp_pl_amd import mesh
    v, f, n, K, poses, _, _ = scene
    m = to_mesh(v, f, n)
    Kt, Pt = torch.from_numpy(K).cuda(), torch.from_numpy(poses).cuda()
    a, za = mesh.vertex_views(m, Kt, Pt, WH, BIAS, near=NEAR, return_zbuffer=True)
    b, zb = mesh.vertex_views(m, Kt, Pt, WH, BIAS, near=NEAR, return_zbuffer=True)
    assert torch.equal(a, b) and torch.equal(za, zb)
    x, y = [mesh.cull_invisible(m, Kt, Pt, WH, BIAS, min_views=5, near=NEAR) for _ in range(2)]
    assert x.faces.shape[0] > 0 and torch.equal(x.faces, y.faces)
    assert torch.equal(x.vertices.view(torch.int32), y.vertices.view(torch.int32)) and torch.equal(x.normals.view(torch.int32), y.normals.view(torch.int32))


def make_model(seed=3):
    from ngp_pl_amd.networks import NGP
    torch.manual_seed(seed)
    m = NGP(scale=0.5).cuda()
    m.register_training_buffers()
    return m


@pytest.fixture
def true_density(monkeypatch):
    """The model's density lattice replaced by the procedural scene's true density, as tests/test_mesh_gpu.py samples it."""
    from ngp_pl_amd import mesh, synthetic as syn

    def volume(model, resolution=512, bounds=None, chunk=0):
        nx, ny, nz = mesh._resolution(resolution)
        xyz = mesh.lattice_points((nx, ny, nz), mesh._bounds(model, bounds))
        return syn.density(xyz).view(nz, ny, nx).contiguous()

    monkeypatch.setattr(mesh, "density_volume", volume)


def test_extract_mesh_with_cull_on_the_true_density(true_density):
    from ngp_pl_amd import mesh, synthetic as syn
    model = make_model()
    res, W = 96, 200
    K, poses = syn.intrinsics(W), syn.hemisphere_poses(12, seed=1)
    plain = mesh.extract_mesh(model, res, 20.0, colors=True)
    again = mesh.extract_mesh(model, res, 20.0, colors=True, cull=None)
    assert torch.equal(plain.faces, again.faces) and torch.equal(plain.vertices.view(torch.int32), again.vertices.view(torch.int32))
    cull = dict(K=K, poses=poses, img_wh=(W, W))
    got = mesh.extract_mesh(model, res, 20.0, colors=True, cull=cull)
    # the cameras are above the horizon: the underside of the base plate goes, the top stays
    assert 0.3 * plain.faces.shape[0] < got.faces.shape[0] < 0.95 * plain.faces.shape[0]
    assert got.colors.shape == got.vertices.shape == got.normals.shape and got.vertices.shape[0] < plain.vertices.shape[0]
    # a subsequence of the vertices, in order: cull the plain mesh with its vertex index riding along as the colour
    lo, hi = mesh._box(model)
    bias = 2.0 * max((b - a) / (res - 1) for a, b in zip(lo, hi))
    ids = torch.arange(plain.vertices.shape[0], device="cuda", dtype=torch.float32)[:, None].repeat(1, 3).contiguous()
    ref = mesh.cull_invisible(mesh.Mesh(plain.vertices, plain.faces, plain.normals, ids), K, poses, (W, W), bias)
    src = ref.colors[:, 0].long()
    assert (src[1:] > src[:-1]).all() and torch.equal(got.faces, ref.faces)
    assert torch.equal(got.vertices.view(torch.int32), plain.vertices[src].view(torch.int32))
    assert torch.equal(got.normals.view(torch.int32), plain.normals[src].view(torch.int32))
    assert torch.allclose(got.colors, plain.colors[src], atol=1e-6)            # evaluated on the kept vertices only
    # the base plate's underside (z = -0.27 less the iso-distance), 4 voxels in from its rim: no camera above the horizon sees it
    def underside(x):
        return (x[:, 2] < -0.27) & (x[:, 0].abs() < 0.30) & (x[:, 1].abs() < 0.18)
    views = mesh.vertex_views(plain, K, poses, (W, W), bias)
    assert underside(plain.vertices).sum() > 100 and (views[underside(plain.vertices)] == 0).all() and not underside(got.vertices).any()
    assert (views[plain.vertices[:, 2] > 0.1] > 0).all()                       # the cabin's and the sphere's tops are seen
    # after the component filter, explicit options
    both = mesh.extract_mesh(model, res, 20.0, keep_largest=1, cull=dict(cull, min_views=2, bias=0.02))
    want = mesh.cull_invisible(mesh.filter_components(mesh.Mesh(plain.vertices, plain.faces, plain.normals), keep_largest=1), K, poses, (W, W), 0.02,
                               min_views=2)
    assert both.colors is None and torch.equal(both.faces, want.faces) and torch.equal(both.vertices.view(torch.int32), want.vertices.view(torch.int32))


def test_cli_cull_cameras(true_density, tmp_path, capsys):
    from ngp_pl_amd import mesh, synthetic as syn
    from tests.test_meshfilter_gpu import read_ply
    model = make_model()
    res, W = 64, 160
    K, poses = syn.intrinsics(W), syn.hemisphere_poses(10, seed=2)
    slim = {"model." + k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt, out, cams = str(tmp_path / "slim.ckpt"), str(tmp_path / "m.ply"), str(tmp_path / "cams.npz")
    torch.save(slim, ckpt)
    np.savez(cams, K=K.numpy(), poses=poses.numpy(), img_wh=np.array([W, W]))
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--cull-cameras", cams, "--cull-min-views", "2", "--cull-bias", "0.03", "--out", out]) == 0
    full = mesh.extract_mesh(model, res)
    want = mesh.cull_invisible(full, K, poses, (W, W), 0.03, min_views=2)
    verts, faces = read_ply(out)
    assert 0 < want.faces.shape[0] < full.faces.shape[0]
    assert np.array_equal(faces, want.faces.cpu().numpy()) and np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), want.vertices.cpu().numpy())
    last = capsys.readouterr().out.strip().splitlines()[-1]
    assert last == "%s: %d vertices, %d faces, %d faces culled as unseen" % (out, len(verts), len(faces), full.faces.shape[0] - len(faces))
    # defaults (one view, two voxels), with the component filter in front
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--keep-largest", "1", "--cull-cameras", cams, "--out", out]) == 0
    verts, faces = read_ply(out)
    want = mesh.extract_mesh(model, res, keep_largest=1, cull=dict(K=K, poses=poses, img_wh=(W, W)))
    assert np.array_equal(faces, want.faces.cpu().numpy())
    last = capsys.readouterr().out.strip().splitlines()[-1]
    assert re_match(last, out, len(verts), len(faces))
    # without the option: the line and the mesh of before
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--out", out]) == 0
    verts, faces = read_ply(out)
    assert np.array_equal(faces, full.faces.cpu().numpy())
    assert capsys.readouterr().out.strip().splitlines()[-1] == "%s: %d vertices, %d faces" % (out, len(verts), len(faces))


def re_match(line, out, n_v, n_f):
    import re
    return re.fullmatch(re.escape("%s: %d vertices, %d faces, " % (out, n_v, n_f)) + r"\d+ components found, 1 kept, \d+ faces culled as unseen", line)
