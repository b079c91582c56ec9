"""GPU: the brick-sparse marching cubes of libngp_meshsparse.so against the dense extractor (bit for bit) and the numpy restatement
(tests/mesh_sparse_reference.py): every cube case, random brick masks, the halo across brick faces, edges and corners, the mask from
the occupancy bitfield, the path through a model, determinism and the empty cases."""
import numpy as np
import pytest
import torch

from tests import mesh_sparse_reference as SR

pytestmark = pytest.mark.gpu


def noise(shape, seed):
    return np.random.RandomState(seed).rand(*shape).astype(np.float32)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def sparse_mc(vol, mask, thr, bounds, **kw):
    from ngp_pl_amd import mesh
    sv = mesh.SparseVolume.from_dense(vol, torch.as_tensor(np.asarray(mask)).cuda())
    return sv, mesh.marching_cubes_sparse(sv, thr, bounds, **kw)


def assert_is_restriction(got, keys, cells, dense, vol_np, thr, mask):
    """got (canonical) is the dense mesh `dense` of the same extractor family restricted to `mask` by the restatement: the same
    integers as the restatement, the same bits as the dense extractor's vertices and normals."""
    keep, used, faces, rkeys, rcell = SR.restrict_indices(vol_np, thr, mask)
    used_t = torch.from_numpy(used).cuda()
    assert np.array_equal(got.faces.cpu().numpy(), faces) and got.faces.dtype == torch.int32
    assert np.array_equal(keys.cpu().numpy(), rkeys) and np.array_equal(cells.cpu().numpy(), rcell)
    assert bits_equal(got.vertices, dense.vertices[used_t]) and bits_equal(got.normals, dense.normals[used_t])
    # and the dense extractor's faces are the restatement's, so `keep` and `used` index the right things
    assert np.array_equal(dense.faces.cpu().numpy()[keep], used[faces])


def test_every_case_with_all_bricks_meshed():
    """(nz, ny, nx) = (22, 13, 17): 3 x 2 x 3 bricks, a partial brick on every axis.  Uniform noise at its median has every cube
    case; points exactly at the threshold are outside."""
    from ngp_pl_amd import mesh
    from tests import mc_reference as R
    vol = noise((22, 13, 17), 11)
    thr = float(np.median(vol))
    vol.reshape(-1)[[5, 400, 1777, 3000, 4861]] = np.float32(thr)
    assert len(np.unique(R.cube_indices(vol, thr))) == 256
    bounds = ((-0.3, -0.5, 0.1), (0.7, 0.25, 1.3))
    v = torch.from_numpy(vol).cuda()
    dense = mesh.marching_cubes(v, thr, bounds)
    sv, got = sparse_mc(v, np.ones(SR.brick_dims(vol.shape), bool), thr, bounds)
    assert sv.n_mesh == sv.n_sample == 18 and dense.faces.shape[0] > 1000
    assert torch.equal(got.vertices, dense.vertices) and torch.equal(got.normals, dense.normals) and torch.equal(got.faces, dense.faces)
    assert bits_equal(got.vertices, dense.vertices) and bits_equal(got.normals, dense.normals)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", [(25, 20, 33), (9, 9, 9)])
def test_random_masks_against_the_restatement(shape, seed):
    from ngp_pl_amd import mesh
    vol = noise(shape, 20 + seed)
    mask = np.random.RandomState(30 + seed).rand(*SR.brick_dims(shape)) < 0.5
    bounds = ((0.0, -1.0, 2.0), (1.0, 0.5, 3.0))
    v = torch.from_numpy(vol).cuda()
    sv, (got, keys, cells) = sparse_mc(v, mask, 0.5, bounds, return_keys=True)
    assert np.array_equal(sv.mask.cpu().numpy(), mask)
    sampled = SR.dilate(mask)
    assert np.array_equal(sv.brick_table.cpu().numpy() >= 0, sampled)
    assert np.array_equal(sv.sample_bricks.cpu().numpy(), np.nonzero(sampled.reshape(-1))[0])
    assert np.array_equal(sv.mesh_bricks.cpu().numpy(), np.nonzero(mask.reshape(-1))[0])
    assert np.array_equal(sv.brick_table.cpu().numpy()[sampled], np.arange(sampled.sum()))
    dense = mesh.marching_cubes(v, 0.5, bounds)
    assert_is_restriction(got, keys, cells, dense, vol, 0.5, mask)
    # the restatement's own vertices and normals: numpy's f32, one rounding per operation, has the device's bits
    rv, rf, rn, _, _ = SR.restrict(vol, 0.5, bounds[0], bounds[1], mask)
    dv = np.abs(got.vertices.cpu().numpy() - rv).max() if len(rv) else 0.0
    dn = np.abs(got.normals.cpu().numpy() - rn).max() if len(rv) else 0.0
    print("shape %r seed %d: %d of %d bricks, V=%d F=%d, against numpy: vertices %.3g normals %.3g" % (
        shape, seed, mask.sum(), mask.size, len(rv), len(rf), dv, dn))
    assert np.array_equal(got.vertices.cpu().numpy(), rv) and np.array_equal(got.normals.cpu().numpy(), rn) and dv == 0 and dn == 0
    # no vertex is unreferenced, keys are strictly increasing after the sort
    n_v = got.vertices.shape[0]
    if n_v:
        assert torch.equal(torch.unique(got.faces.long()), torch.arange(n_v, device="cuda"))
        assert (keys[1:] > keys[:-1]).all() and (cells[1:] >= cells[:-1]).all()
    else:
        assert not mask.any() or got.faces.shape[0] == 0


def sphere(n, centre, radius):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return (radius - d).astype(np.float32)


@pytest.mark.parametrize("centre", [(16, 16, 16), (8, 8, 8)])
def test_halo_only_the_bricks_with_a_crossed_cell_are_meshed(centre):
    """A sphere of radius 9.3 voxels round the lattice point eight bricks share, on a 27^3 lattice (4 bricks per axis, the last one
    partial): its surface crosses brick faces, edges and the corner, and the normals of vertices near them read points of bricks
    that are sampled but not meshed.  Round (8, 8, 8) the sphere leaves the lattice: the differences at the border are one-sided."""
    from ngp_pl_amd import mesh
    from tests import mc_reference as R
    vol = sphere(27, centre, 9.3)
    cube = R.cube_indices(vol, 0.0)
    crossed = (cube != 0) & (cube != 255)
    mask = np.zeros(SR.brick_dims(vol.shape), bool)
    cz, cy, cx = np.nonzero(crossed)
    mask[cz // 8, cy // 8, cx // 8] = True
    assert 8 <= mask.sum() < mask.size
    assert mask[centre[2] // 8 - 1:centre[2] // 8 + 1, centre[1] // 8 - 1:centre[1] // 8 + 1, centre[0] // 8 - 1:centre[0] // 8 + 1].all()
    bounds = ((-1.0, -1.0, -1.0), (1.0, 1.5, 2.0))
    v = torch.from_numpy(vol).cuda()
    dense = mesh.marching_cubes(v, 0.0, bounds)
    sv, got = sparse_mc(v, mask, 0.0, bounds)
    assert sv.n_mesh == mask.sum() and sv.n_sample == SR.dilate(mask).sum() and sv.n_sample > sv.n_mesh
    assert got.faces.shape[0] == dense.faces.shape[0] > 1000
    assert torch.equal(got.faces, dense.faces) and bits_equal(got.vertices, dense.vertices) and bits_equal(got.normals, dense.normals)
    if centre == (8, 8, 8):                               # vertices on the lattice's border planes exist
        assert (got.vertices[:, 0] == -1.0).any() and (got.vertices[:, 2] == -1.0).any()
    # the points outside the sampled bricks do not matter: poison them
    sampled = SR.dilate(mask)
    poison = vol.copy()
    bz, by, bx = np.nonzero(~sampled)
    for z, y, x in zip(bz, by, bx):
        poison[8 * z:8 * z + 8, 8 * y:8 * y + 8, 8 * x:8 * x + 8] = np.nan
    if len(bz):
        again = sparse_mc(torch.from_numpy(poison).cuda(), mask, 0.0, bounds)[1]
        assert torch.equal(again.faces, dense.faces) and bits_equal(again.vertices, dense.vertices) and bits_equal(again.normals, dense.normals)


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


def test_many_bricks_and_a_partial_mask():
    """(nz, ny, nx) = (130, 128, 129): 17 x 16 x 17 = 4624 bricks, three blocks of the index scan and more sample slots than the
    scan has threads; a mask of the crossed bricks and a few more."""
    from ngp_pl_amd import mesh
    from tests import mc_reference as R
    vol = smooth_volume((130, 128, 129), 3)
    cube = R.cube_indices(vol, 0.6)
    mask = np.random.RandomState(4).rand(*SR.brick_dims(vol.shape)) < 0.01
    cz, cy, cx = np.nonzero((cube != 0) & (cube != 255))
    mask[cz // 8, cy // 8, cx // 8] = True
    bounds = ((-0.3, -0.5, 0.1), (0.7, 0.25, 1.3))
    v = torch.from_numpy(vol).cuda()
    dense = mesh.marching_cubes(v, 0.6, bounds)
    sv, got = sparse_mc(v, mask, 0.6, bounds)
    assert 1024 < sv.n_sample < mask.size and sv.n_mesh == mask.sum()
    assert np.array_equal(sv.sample_bricks.cpu().numpy(), np.nonzero(SR.dilate(mask).reshape(-1))[0])
    assert torch.equal(got.faces, dense.faces) and bits_equal(got.vertices, dense.vertices) and bits_equal(got.normals, dense.normals)


def occupancy_cases(scale):
    full = ((-scale,) * 3, (scale,) * 3)
    # bricks of the sub-box, grown, reach past +-0.5: the box of cascade 0 (with one cascade: past the only box, the fallback)
    sub = ((-0.5, -0.4, -0.3), (0.5, 0.3, 0.45)) if scale <= 0.5 else ((-0.7, -0.45, -0.3), (0.45, 0.6, 0.52))
    small = ((0.11, -0.2, 0.3), (0.14, -0.17, 0.33))     # ten lattice spacings fit one occupancy cell: one thread per brick
    return [(res, box) for res in (40, (70, 33, 18)) for box in (full, sub)] + [(40, small)]


@pytest.mark.parametrize("scale,cascades", [(0.5, 1), (2.0, 3)])
def test_mask_from_the_bitfield(scale, cascades):
    from ngp_pl_amd import mesh
    from ngp_pl_amd.networks import NGP
    model = NGP(scale=scale).cuda()
    G = model.grid_size
    assert model.cascades == cascades and G == 128
    g = np.random.RandomState(5)
    cells = [(k, c0, c1, c2) for k in range(cascades) for c0 in (0, G - 1) for c1 in (0, G - 1) for c2 in (0, G - 1)]
    cells += [(int(g.randint(cascades)),) + tuple(int(c) for c in g.randint(0, G, 3)) for _ in range(12)]
    cells += [(0, 78, 38, 102), (0, 64, 64, 64)]         # inside the small box, and at the centre
    bits = SR.set_bits(cascades, G, cells)
    model.density_bitfield.copy_(torch.from_numpy(bits))
    grids = SR.occupancy_grids(bits, cascades, G)
    seen = set()
    for res, (lo, hi) in occupancy_cases(scale):
        nx, ny, nz = (res,) * 3 if isinstance(res, int) else res
        for margin in (0, 1, 3):
            got = mesh.brick_mask_from_occupancy(model, res, (lo, hi), margin_voxels=margin)
            want = SR.occupancy_mask(bits, cascades, G, scale, (nz, ny, nx), lo, hi, margin, grids=grids)
            assert got.dtype == torch.bool and got.is_cuda and tuple(got.shape) == want.shape
            assert np.array_equal(got.cpu().numpy(), want), (res, lo, hi, margin)
            seen.add((bool(want.any()), bool(want.all())))
    assert (True, False) in seen
    assert mesh.brick_mask_from_occupancy(model, 40).shape == (5, 5, 5)         # the defaults: the model's box, one voxel
    model.density_bitfield.zero_()
    assert not mesh.brick_mask_from_occupancy(model, 40).any()
    with pytest.raises(ValueError):
        mesh.brick_mask_from_occupancy(model, 40, margin_voxels=-1)


def make_model(seed=3):
    from ngp_pl_amd.networks import NGP
    torch.manual_seed(seed)
    m = NGP(scale=0.5).cuda()
    m.register_training_buffers()
    with torch.no_grad():
        m.xyz_encoder.params.normal_(0, 0.5)             # a non-trivial field without training
        m.xyz_encoder._half.invalidate()
    return m


def test_through_a_model():
    from ngp_pl_amd import mesh
    model = make_model()
    res, lo, hi = (24, 20, 16), (-0.5, -0.4, -0.3), (0.5, 0.3, 0.45)
    nx, ny, nz = res
    nb = SR.brick_dims((nz, ny, nx))
    all_true = torch.ones(nb, dtype=torch.bool, device="cuda")
    some = torch.from_numpy(np.random.RandomState(6).rand(*nb) < 0.4).cuda()
    dense_vol = mesh.density_volume(model, res, (lo, hi))
    every = mesh.lattice_points(res, (lo, hi))
    for mask, chunk in ((all_true, 5), (some, 4), (all_true, 1 << 13)):
        sv = mesh.sparse_density_volume(model, res, (lo, hi), mask=mask, chunk_bricks=chunk)
        assert sv.n_sample % chunk != 0 and (sv.n_sample > 2 * chunk or chunk > 100)      # several chunks, a ragged last one
        # the points kernel against lattice_points at the same lattice indices (clamped past the lattice's end)
        z, y, x, real = sv._coords()
        xyz = mesh.sparse_lattice_points(sv, (lo, hi))
        assert torch.equal(xyz, every[((z * ny + y) * nx + x).reshape(-1)])
        assert not real.all() and torch.equal(mesh.sparse_lattice_points(sv, (lo, hi), 2, 3), xyz[2 * 512:5 * 512])
        with torch.no_grad():
            want = model.density(xyz).view(-1, 512)
        assert torch.allclose(sv.pool, want, rtol=1e-3, atol=1e-6), (sv.pool - want).abs().max()
        differ = int((sv.pool.view(torch.int32) != dense_vol[z, y, x].view(torch.int32))[real].sum())
        print("chunk_bricks=%d: %d sample slots, %d of %d sampled lattice points differ bitwise from density_volume" % (
            chunk, sv.n_sample, differ, int(real.sum())))
        # marching cubes on the pool against the dense extractor on the same sigmas
        thr = float(sv.pool[real].median())
        rebuilt = sv.to_dense()
        got, keys, cells = mesh.marching_cubes_sparse(sv, thr, (lo, hi), return_keys=True)
        dense = mesh.marching_cubes(rebuilt, thr, (lo, hi))
        assert got.faces.shape[0] > 500
        assert_is_restriction(got, keys, cells, dense, rebuilt.cpu().numpy(), thr, mask.cpu().numpy())
    thr = float(dense_vol.median())
    a = mesh.extract_mesh(model, res, thr, (lo, hi))
    b = mesh.extract_mesh(model, res, thr, (lo, hi), sparse=dict(mask=all_true))
    assert a.faces.shape[0] == b.faces.shape[0] > 500 and a.vertices.shape == b.vertices.shape
    # the later stages take the sparse mesh as they take the dense one
    c = mesh.extract_mesh(model, res, thr, (lo, hi), sparse=dict(mask=all_true), colors=True, keep_largest=1)
    d = mesh.extract_mesh(model, res, thr, (lo, hi), colors=True, keep_largest=1)
    assert c.faces.shape == d.faces.shape and c.colors.shape == c.vertices.shape
    # the occupancy grid of an untrained model is empty: nothing is sampled, the mesh is empty
    e = mesh.extract_mesh(model, res, thr, (lo, hi), sparse=True)
    assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3)
    model.density_bitfield.fill_(255)
    f = mesh.extract_mesh(model, res, thr, (lo, hi), sparse=dict(margin_voxels=0))
    assert f.faces.shape[0] == a.faces.shape[0]


def test_deterministic_and_edge_cases():
    from ngp_pl_amd import mesh
    vol = noise((25, 20, 33), 40)
    mask = np.random.RandomState(41).rand(*SR.brick_dims(vol.shape)) < 0.5
    v = torch.from_numpy(vol).cuda()
    runs = [sparse_mc(v, mask, 0.5, None, canonical=False, return_keys=True)[1] for _ in range(2)]
    (a, ka, ca), (b, kb, cb) = runs
    assert a.faces.shape[0] > 1000 and torch.equal(a.faces, b.faces) and torch.equal(ka, kb) and torch.equal(ca, cb)
    assert bits_equal(a.vertices, b.vertices) and bits_equal(a.normals, b.normals)
    # the raw order: brick by brick in ascending brick number, then local order
    nz, ny, nx = vol.shape
    nbz, nby, nbx = SR.brick_dims(vol.shape)

    def order(lin):
        x, y, z = lin % nx, (lin // nx) % ny, lin // (nx * ny)
        return (((z // 8) * nby + y // 8) * nbx + x // 8) * 512 + ((z % 8) * 8 + y % 8) * 8 + x % 8

    ko = order(ka // 3) * 3 + ka % 3
    assert (ko[1:] > ko[:-1]).all() and (order(ca)[1:] >= order(ca)[:-1]).all() and not (ka[1:] > ka[:-1]).all()
    # the canonical form is the raw one sorted
    c, kc, cc = sparse_mc(v, mask, 0.5, None, return_keys=True)[1]
    assert torch.equal(kc, torch.sort(ka)[0]) and bits_equal(c.vertices, a.vertices[torch.sort(ka)[1]])
    assert bits_equal(c.vertices[c.faces.long()], a.vertices[a.faces.long()][torch.sort(ca, stable=True)[1]])
    # nothing meshed, and nothing crossed
    e = sparse_mc(v, np.zeros_like(mask), 0.5, None, return_keys=True)[1]
    assert e[0].vertices.shape == (0, 3) and e[0].normals.shape == (0, 3) and e[0].faces.shape == (0, 3) and e[1].shape == e[2].shape == (0,)
    for fill in (0.0, 1.0):
        flat = torch.full((9, 10, 11), fill, device="cuda")
        for canonical in (True, False):
            m = sparse_mc(flat, np.ones((2, 2, 2), bool), 0.5, None, canonical=canonical)[1]
            assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.faces.dtype == torch.int32
    with pytest.raises(ValueError, match="sparse and tsdf"):
        mesh.extract_mesh(None, 16, sparse=True, tsdf=dict(K=np.eye(3), poses=np.zeros((1, 3, 4)), img_wh=(8, 8)))
