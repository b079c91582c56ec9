"""GPU: marching cubes of libngp_mesh.so against the numpy restatement (tests/mc_reference.py), topology on every cube case,
analytic shapes, the procedural scene's true density, the model path (lattice sampler, trained field, vertex colours) and
determinism."""
import math

import numpy as np
import pytest
import torch

from ngp_pl_amd import synthetic as syn
from tests import mc_reference as R

pytestmark = pytest.mark.gpu


def smooth_volume(shape, seed):
    """Sum of a few random Gaussian blobs: a smooth field with several iso-surface components."""
    g = np.random.RandomState(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.linspace(0, 1, nz), np.linspace(0, 1, ny), np.linspace(0, 1, nx), indexing="ij")
    v = np.zeros(shape)
    for _ in range(6):
        c, s, a = g.rand(3), 0.08 + 0.12 * g.rand(), 0.5 + g.rand()
        v += a * np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * s * s))
    return v.astype(np.float32)


def gpu_mc(vol, thr, lo, hi):
    from ngp_pl_amd import mesh
    m = mesh.marching_cubes(torch.from_numpy(vol).cuda(), thr, (lo, hi))
    return m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.normals.cpu().numpy()


@pytest.mark.parametrize("shape,seed", [((48, 48, 48), 0), ((72, 56, 40), 1), ((33, 65, 17), 2), ((130, 128, 128), 3)])
def test_exact_against_numpy_restatement(shape, seed):
    """(nz, ny, nx) = (72, 56, 40) is the non-cubic 40 x 56 x 72 lattice.  (130, 128, 128) has 1040 bricks of 2048 points: the
    one-workgroup scan of the brick counts takes a second brick per thread."""
    vol = smooth_volume(shape, seed)
    lo, hi = (-0.3, -0.5, 0.1), (0.7, 0.25, 1.3)
    v, f, n = gpu_mc(vol, 0.6, lo, hi)
    rv, rf, rn, _ = R.marching_cubes(vol, 0.6, lo, hi)
    assert len(rf) > 100
    assert f.dtype == np.int32 and np.array_equal(f, rf)
    ext = max(b - a for a, b in zip(lo, hi))
    assert v.shape == rv.shape and np.abs(v - rv).max() <= 1e-6 * ext
    assert np.abs(n - rn).max() <= 1e-5


def test_watertight_and_oriented_on_every_case():
    g = np.random.RandomState(5)
    vol = g.rand(64, 64, 64).astype(np.float32)
    vol[[0, -1]] = 0
    vol[:, [0, -1]] = 0
    vol[:, :, [0, -1]] = 0
    v, f, _ = gpu_mc(vol, 0.5, (0, 0, 0), (1, 1, 1))
    cube = R.cube_indices(vol, 0.5)
    hist = np.bincount(cube.reshape(-1), minlength=256)
    assert (hist[1:255] > 0).all(), np.nonzero(hist[1:255] == 0)
    assert len(v) == (f.max() + 1) and R.is_closed_oriented(f)
    rv, rf, _, _ = R.marching_cubes(vol, 0.5, (0, 0, 0), (1, 1, 1))
    assert np.array_equal(f, rf)


def _centered(n, lo=-1.0, hi=1.0):
    x = np.linspace(lo, hi, n).astype(np.float32)
    z, y, x = np.meshgrid(x, x, x, indexing="ij")
    return x, y, z


def test_sphere():
    n = 128
    x, y, z = _centered(n, -64.0, 64.0)          # spacing 128/127 per voxel
    r = 40.0
    vol = (r - np.sqrt(x * x + y * y + z * z)).astype(np.float32)
    v, f, nrm = gpu_mc(vol, 0.0, (-64, -64, -64), (64, 64, 64))
    assert R.is_closed_oriented(f) and R.euler(v, f) == 2
    assert abs(R.area(v, f) / (4 * math.pi * r * r) - 1) < 0.01
    vol_ = R.signed_volume(v, f)
    assert vol_ > 0 and abs(vol_ / (4 / 3 * math.pi * r ** 3) - 1) < 0.01
    radial = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert (np.sum(radial * nrm, 1) > 0.99).mean() > 0.99          # normals point outward


def test_torus():
    x, y, z = _centered(96)
    R0, r0 = 0.55, 0.2
    vol = (r0 - np.sqrt((np.sqrt(x * x + y * y) - R0) ** 2 + z * z)).astype(np.float32)
    v, f, _ = gpu_mc(vol, 0.0, (-1, -1, -1), (1, 1, 1))
    assert R.is_closed_oriented(f) and R.euler(v, f) == 0 and R.signed_volume(v, f) > 0


def test_procedural_scene_true_density():
    """Every vertex lies on a lattice edge that straddles the iso-point, and the SDF is 1-Lipschitz: its signed distance is within
    one spacing of the iso-distance."""
    from ngp_pl_amd import mesh
    n = 256
    lo, hi = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
    xyz = mesh.lattice_points(n, (lo, hi))
    vol = syn.density(xyz).view(n, n, n).contiguous()
    m = mesh.marching_cubes(vol, 20.0, (lo, hi))
    assert m.faces.shape[0] > 10000
    h = 1.0 / (n - 1)
    p = 20.0 / syn.SIGMA_INSIDE
    sd_iso = -syn.EDGE * math.log(p / (1 - p))
    err = (syn.signed_distance(m.vertices.double()) - sd_iso).abs().max().item()
    assert err <= h * (1 + 1e-3), (err, h)
    assert R.is_closed_oriented(m.faces.cpu().numpy())


def make_model(seed=0):
    from ngp_pl_amd.networks import NGP
    torch.manual_seed(seed)
    m = NGP(scale=0.5).cuda()
    m.register_training_buffers()
    return m


def test_density_volume_matches_model_density():
    from ngp_pl_amd import mesh
    model = make_model(3)
    with torch.no_grad():
        model.xyz_encoder.params.normal_(0, 0.5)         # a non-trivial field without training
        model.xyz_encoder._half.invalidate()
    res, lo, hi = (24, 20, 16), (-0.5, -0.4, -0.3), (0.5, 0.3, 0.45)
    vol = mesh.density_volume(model, res, (lo, hi), chunk=1000)          # several chunks, a ragged last one
    nx, ny, nz = res
    # the documented lattice in f32: h = (hi - lo) / (n - 1), point = lo + i * h (two roundings, as the sampler computes it)
    lo_t, hi_t = torch.tensor(lo, device="cuda"), torch.tensor(hi, device="cuda")
    h = (hi_t - lo_t) / torch.tensor([nx - 1.0, ny - 1.0, nz - 1.0], device="cuda")
    kk, jj, ii = torch.meshgrid(*[torch.arange(k, device="cuda", dtype=torch.float32) for k in (nz, ny, nx)], indexing="ij")
    idx = torch.stack([ii, jj, kk], -1).reshape(-1, 3)
    xyz = (lo_t + idx * h).contiguous()
    assert torch.equal(xyz, mesh.lattice_points(res, (lo, hi)))
    with torch.no_grad():
        want = model.density(xyz).view(nz, ny, nx)
    assert vol.shape == (nz, ny, nx)
    assert torch.allclose(vol, want, rtol=1e-3, atol=1e-6), (vol - want).abs().max()
    with pytest.raises(ValueError):
        mesh.density_volume(model, 8, ((-0.6, -0.5, -0.5), (0.5, 0.5, 0.5)))


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


def test_trained_model_mesh_lies_on_the_true_surface(trained):
    """2 000 native steps of 4096 rays, extract_mesh at 256^3 (voxel h = 1/255 of the box), |signed distance - iso distance| of the
    vertices.  Measured on an MI355X (training is bit-reproducible): V = 73 826, F = 122 744, median 12.47 h, p95 57.2 h.  The
    median is NOT within one voxel: the cameras sit above the horizon and 2 000 steps constrain the density only along the
    rays that reach the surface, so the iso-20 set also has sheets inside the solids and under the floor.  The bounds below
    (median < 16 h, p95 < 72 h) pin that measured state with margin, so a regression of the lattice or the extraction shows."""
    from ngp_pl_amd import mesh
    m = mesh.extract_mesh(trained, 256)
    assert m.faces.shape[0] > 10000
    p = 20.0 / syn.SIGMA_INSIDE
    sd_iso = -syn.EDGE * math.log(p / (1 - p))
    d = (syn.signed_distance(m.vertices.double()) - sd_iso).abs()
    h = 1.0 / 255
    med, p95 = d.median().item() / h, torch.quantile(d[torch.randperm(len(d), device=d.device)[:1000000]], 0.95).item() / h
    print("trained mesh: V=%d F=%d median %.3f voxels p95 %.3f voxels" % (m.vertices.shape[0], m.faces.shape[0], med, p95))
    assert med < 16.0 and p95 < 72.0, (med, p95)


def test_vertex_colors_are_the_field_seen_along_minus_normal(trained):
    from ngp_pl_amd import mesh
    m = mesh.extract_mesh(trained, 64, colors=True)
    assert m.colors.shape == m.vertices.shape and m.vertices.shape[0] > 100
    d = -m.normals
    d[(m.normals == 0).all(1)] = torch.tensor([0.0, 0.0, 1.0], device="cuda")
    with torch.no_grad():
        _, rgb = trained(m.vertices, d.contiguous())
    assert torch.allclose(m.colors, rgb.float(), atol=1e-6)
    assert (m.colors >= 0).all() and (m.colors <= 1).all()


def test_deterministic_and_edge_cases():
    from ngp_pl_amd import mesh
    vol = torch.from_numpy(smooth_volume((80, 70, 60), 7)).cuda()
    a = mesh.marching_cubes(vol, 0.6, ((0, 0, 0), (1, 1, 1)))
    b = mesh.marching_cubes(vol, 0.6, ((0, 0, 0), (1, 1, 1)))
    assert torch.equal(a.faces, b.faces)
    assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32)) and torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32))
    for fill in (0.0, 1.0):
        e = mesh.marching_cubes(torch.full((9, 10, 11), fill, device="cuda"), 0.5)
        assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3)
    # values exactly at the threshold are outside (strict comparison) and give no NaN
    q = torch.from_numpy(np.random.RandomState(3).randint(0, 3, (20, 20, 20)).astype(np.float32)).cuda()
    m = mesh.marching_cubes(q, 1.0, ((0, 0, 0), (1, 1, 1)))
    assert m.faces.shape[0] > 0 and torch.isfinite(m.vertices).all() and torch.isfinite(m.normals).all()
    rv, rf, rn, _ = R.marching_cubes(q.cpu().numpy(), 1.0, (0, 0, 0), (1, 1, 1))
    assert np.array_equal(m.faces.cpu().numpy(), rf) and np.abs(m.vertices.cpu().numpy() - rv).max() <= 1e-6


def test_other_device_is_honoured():
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU on this box")
    from ngp_pl_amd import mesh
    vol = torch.from_numpy(smooth_volume((30, 30, 30), 9))
    m1 = mesh.marching_cubes(vol.to("cuda:1"), 0.6, ((0, 0, 0), (1, 1, 1)))
    m0 = mesh.marching_cubes(vol.to("cuda:0"), 0.6, ((0, 0, 0), (1, 1, 1)))
    assert m1.faces.device.index == 1 and torch.equal(m1.faces.cpu(), m0.faces.cpu())
    assert torch.equal(m1.vertices.cpu(), m0.vertices.cpu())
