"""GPU: libngp_meshnormal.so against the numpy restatement (tests/mesh_normal_reference.py), as integer words: the transferred
normals, squared distances, faces and barycentric pairs against the brute force over every face, for query counts round the wave
and the workgroup, queries on cell faces, edges and corners and outside the grid, on the exit boundaries and at the cap, on ties
and under a permutation of the faces, with and without the orientation test, with degenerate faces, normals and queries; the
agreement with closest_on_mesh; chunks and repeated runs; the shading; and bake_normal_map, render_textured, extract_mesh and the
CLI end to end."""
import json
import os

import numpy as np
import pytest
import torch

from tests import mesh_distance_reference as DR
from tests import mesh_normal_reference as NR
from tests import mesh_texture_reference as TR
from tests.test_meshtex_gpu import bits, make_model, same_mesh, true_density  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
CELL = 0.25
REACH = 0.6


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_mesh(v, f, vn=None):
    from ngp_pl_amd import mesh
    return mesh.Mesh(dev(np.asarray(v, F).reshape(-1, 3)), dev(np.asarray(f, np.int32).reshape(-1, 3)), None if vn is None else dev(np.asarray(vn, F)))


def run(q, m, valid, detail, max_dist, oriented=True, grid=None, debug=False):
    """ngp_meshnormal_transfer through the Python layer, with the squared distance as the library writes it."""
    from ngp_pl_amd import mesh
    v, f, vn = detail
    d = to_mesh(v, f, vn)
    if grid is None:
        grid = mesh.distance_grid(d, cell=CELL)
    valid = np.ones(len(q), np.uint8) if valid is None else valid
    return mesh._transfer(dev(np.asarray(q, F)), dev(np.asarray(m, F)), dev(np.asarray(valid, np.uint8)), d.vertices, d.faces, d.normals, grid,
                          float(F(max_dist)), oriented, debug=debug)


def same(got, want):
    n, d2, face, bary = got[:4]
    assert np.array_equal(face.cpu().numpy(), want[2]), int((face.cpu().numpy() != want[2]).sum())
    assert np.array_equal(bits(d2), bits(want[1])), int((bits(d2) != bits(want[1])).sum())
    assert np.array_equal(bits(bary), bits(want[3]))
    assert np.array_equal(bits(n), bits(want[0])), int((bits(n) != bits(want[0])).any(1).sum())


@pytest.fixture(scope="module")
def lat():
    return NR.lattice()


@pytest.fixture(scope="module")
def grid(lat):
    from ngp_pl_amd import mesh
    return mesh.distance_grid(to_mesh(*lat), cell=CELL)


@pytest.fixture(scope="module")
def queries(lat, grid):
    """1 000 queries round the two sheets: inside cells, on cell faces, edges and corners, beyond every side of the grid, with
    normals that point everywhere (and straight up and down), a few that are not valid or not finite; and the brute force of
    both kinds for them, computed once."""
    v, f, vn = lat
    o, cell, dims = np.array(grid.origin, F), F(grid.cell), grid.dims
    assert min(dims) >= 2 and float(cell) == CELL
    g = np.random.RandomState(31)
    lo, hi = o, o + np.array(dims, F) * cell
    q = [g.uniform(lo, hi, (600, 3))]
    corner = lambda i, j, k: o + np.array([i, j, k], F) * cell
    for _ in range(30):
        i, j, k = (g.randint(0, n + 1) for n in dims)
        h = g.uniform(0, 1, 3).astype(F) * cell
        q += [corner(i, j, k)[None], (corner(i, j, k) + h * np.array([0, 1, 1], F))[None], (corner(i, j, k) + h * np.array([0, 0, 1], F))[None],
              (corner(i, j, k) + h * np.array([1, 0, 1], F))[None]]
    ext = hi - lo
    for axis in range(3):
        for side in (-1, 1):
            p = g.uniform(lo, hi, (8, 3))
            p[:, axis] = (lo[axis] - g.uniform(0.01, 0.5, 8) * ext[axis]) if side < 0 else (hi[axis] + g.uniform(0.01, 0.5, 8) * ext[axis])
            q.append(p)
    q += [(hi + 0.3 * ext)[None], (lo - 1.7 * ext)[None], (hi + 40 * ext)[None]]
    q = np.concatenate([np.asarray(x, np.float64).reshape(-1, 3) for x in q])
    q = np.concatenate([q, g.uniform(lo, hi, (1000 - len(q), 3))]).astype(F)
    m = g.normal(size=(1000, 3)).astype(F)
    m[::7], m[3::7] = F([0, 0, 1]), F([0, 0, -2])
    valid = np.ones(1000, np.uint8)
    valid[[5, 500]] = 0
    q[6], q[501], q[777] = F([np.nan, 0, 0]), F([0, np.inf, 0.1]), F([0.1, 0.2, -np.inf])
    m[8], m[9], m[10] = F([0, 0, 0]), F([np.nan, 1, 0]), F([np.inf, 0, 0])
    want = {o_: NR.transfer_f32(q, m, valid, v, f, vn, REACH, o_) for o_ in (True, False)}
    hits = want[True][2] >= 0
    assert hits.sum() > 200 and (~hits).sum() > 50 and (want[True][2] != want[False][2]).sum() > 100        # orientation decides many of them
    return q, m, valid, want


# ---- the query against the brute force


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_words_equal_the_brute_force_minimum(lat, grid, queries, n):
    q, m, valid, want = queries
    pick = np.arange(1000) if n == 1000 else np.random.RandomState(n).permutation(1000)[:n]
    for oriented in (True, False):
        got = run(q[pick], m[pick], valid[pick], lat, REACH, oriented, grid, debug=True)
        same(got, tuple(w[pick] for w in want[oriented]))
        dbg = got[4].cpu().numpy()
        dead = (valid[pick] == 0) | ~np.isfinite(q[pick]).all(1)
        assert not dbg[dead].any() and (dbg[~dead, 0] >= 1).all() and dbg[:, 0].max() <= NR.MAX_SHELLS + 2
        assert not got[0].cpu().numpy()[dead].any() and (got[2].cpu().numpy()[dead] == -1).all()
    if n == 1000:                                               # two runs, the same bits
        same(run(q, m, valid, lat, REACH, True, grid), want[True])


def test_four_further_grids_give_the_same_words(lat, queries):
    from ngp_pl_amd import mesh
    q, m, valid, want = queries
    v = lat[0]
    d = to_mesh(*lat)
    lo, ext = v.min(0), v.max(0) - v.min(0)
    grids = [mesh.distance_grid(d, cell=float(ext.max()) * 1.01, origin=lo - 0.005 * ext, dims=(1, 1, 1)),
             mesh.distance_grid(d, cell=float(ext.max()) / 1.9, origin=lo - 0.013 * ext, dims=(2, 3, 1)),
             mesh.distance_grid(d, cell=0.17, origin=lo + 0.21 * ext, dims=(3, 4, 2)),                   # covers a corner of the target only
             mesh.distance_grid(d, cell=0.077)]
    assert grids[0].dims == (1, 1, 1) and min(grids[3].dims) >= 5 and all(REACH <= 8 * g.cell for g in grids)
    for g in grids:
        for oriented in (True, False):
            same(run(q, m, valid, lat, REACH, oriented, g), want[oriented])


def test_exit_boundaries_and_the_cap(lat, grid):
    """Straight over the upper sheet (it faces +z, at z = 0.3) the distance is exact: queries at r cells above it, give or take a
    few ulps and the slack, sit on the distance exit of shell r; with max_dist = r cells they sit on the max_dist exit and on the
    reach itself; max_dist = 8 cells is the cap, accepted, and one ulp more is refused."""
    from ngp_pl_amd import _lib
    v, f, vn = lat
    top = float(v[:, 2].max())
    o, dims = np.array(grid.origin, F), grid.dims
    mag = max(np.abs(o).max(), np.abs(o + np.array(dims, F) * F(CELL)).max())
    q = []
    for r in (1, 2, 3, 8):
        z = float(F(top) + F(r) * F(CELL))
        ulp, s = float(np.spacing(F(z))), float(DR.slack(max(z, mag)))
        q += [[0.1, -0.2, z + step] for step in (-3 * ulp, -2 * ulp, -ulp, 0.0, ulp, 2 * ulp, 3 * ulp, -s, s, -s - ulp, s + ulp)]
        q += [[0.1, -0.2, -(z - top) + step] for step in (-ulp, 0.0, ulp)]                                # and under the lower sheet
    q = np.array(q, F)
    up = np.tile(F([0, 0, 1]), (len(q), 1))
    for m in (up, -up):
        for oriented in (True, False):
            for max_dist in (CELL, 2 * CELL, 3 * CELL, float(np.nextafter(F(3 * CELL), F(0))), 8 * CELL, 1.9):
                want = NR.transfer_f32(q, m, None, v, f, vn, max_dist, oriented)
                same(run(q, m, None, lat, max_dist, oriented, grid), want)
    full = NR.transfer_f32(q, up, None, v, f, vn, 8 * CELL, True)
    assert (full[2] >= 0).sum() >= 30 and (full[2] < 0).sum() >= 5                                        # both sides of the cap's reach
    with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
        run(q, up, None, lat, float(np.nextafter(F(8 * CELL), F(np.inf))), True, grid)
    with pytest.raises(_lib.NgpError, match="NGP_EINVAL"):
        run(q, up, None, lat, float("inf"), False, grid)


def test_ties_go_to_the_smaller_index_and_permutations_agree(lat, queries):
    v, f, vn = lat
    q, m, valid, _ = queries
    f2 = np.concatenate([f, f[100:101], f[3:4]])                 # two faces once more: bit-equal ties
    over = v[f[100]].mean(0) + F([0, 0, 0.1])
    under = v[f[3]].mean(0) - F([0, 0, 0.1])
    q = np.concatenate([q[:300], np.stack([over, under])]).astype(F)
    m = np.concatenate([m[:300], F([[0, 0, 1], [0, 0, -1]])])
    valid = np.ones(len(q), np.uint8)
    want = NR.transfer_f32(q, m, valid, v, f2, vn, REACH, True)
    assert want[2][-2:].tolist() == [100, 3] and not (want[2] >= len(f)).any()
    same(run(q, m, valid, (v, f2, vn), REACH, True), want)
    perm = np.random.RandomState(32).permutation(len(f2))        # new face j is old face perm[j]
    fp = f2[perm]
    for oriented in (True, False):
        got = run(q, m, valid, (v, fp, vn), REACH, oriented)
        expect = NR.transfer_f32(q, m, valid, v, fp, vn, REACH, oriented)
        same(got, expect)
        assert np.array_equal(bits(got[1]), bits(NR.transfer_f32(q, m, valid, v, f2, vn, REACH, oriented)[1]))     # the distance does not depend on the order


# ---- eligibility


def test_the_thin_wall_oriented_and_not():
    wall = NR.thin_wall()
    p, m = F([[0.3, 0.4, 0.006]]), F([[0, 0, -1]])
    from ngp_pl_amd import mesh
    g = mesh.distance_grid(to_mesh(*wall), cell=0.5)
    n, d2, face, _, _ = run(p, m, None, wall, 1.0, False, g)
    e = F(0.006) - F(0.01)
    assert face.item() in (2, 3) and d2.item() == float(e * e) and n[0].tolist() == [0, 0, 1]
    n, d2, face, _, _ = run(p, m, None, wall, 1.0, True, g)
    assert face.item() in (0, 1) and d2.item() == float(F(0.006) * F(0.006)) and n[0].tolist() == [0, 0, -1]
    n, d2, face, bary, _ = run(p, m, None, wall, 0.005, True, g)
    assert face.item() == -1 and d2.item() == float("inf") and n[0].tolist() == [0, 0, -1] and bary[0].tolist() == [0, 0]
    for oriented, max_dist in ((True, 1.0), (False, 1.0), (True, 0.005), (False, 0.005)):
        same(run(p, m, None, wall, max_dist, oriented, g), NR.transfer_f32(p, m, None, *wall, max_dist, oriented))


def test_the_only_eligible_face_in_shell_three_and_none_at_all(lat):
    """Over the lower sheet, which faces down, a query that looks up finds nothing near; its one eligible face is a small triangle
    three cells away.  A query that looks along x finds no eligible face at all (every face normal is +-z): a miss after the
    bounded walk the cap gives, read from the debug output."""
    from ngp_pl_amd import mesh
    v, f, vn = lat
    low = f[:72]                                                 # the sheet at z = 0, facing -z
    tri_v = F([[0.0, 0.0, 0.8], [0.1, 0.0, 0.8], [0.0, 0.1, 0.8]])
    v2 = np.concatenate([v, tri_v])
    vn2 = np.concatenate([vn, np.tile(F([0, 0, 1]), (3, 1))])
    f2 = np.concatenate([low, np.array([[len(v), len(v) + 1, len(v) + 2]], np.int32)])
    detail = (v2, f2, vn2)
    g = mesh.distance_grid(to_mesh(*detail), cell=CELL, origin=(-3.0, -3.0, -3.0), dims=(24, 24, 24))
    q = F([[0.02, 0.03, 0.03]])
    cz = DR.cell_of(0.03, -3.0, CELL, 24)
    assert DR.cell_of(0.8, -3.0, CELL, 24) - cz == 3
    got = run(q, F([[0, 0, 1]]), None, detail, 4 * CELL, True, g, debug=True)
    same(got, NR.transfer_f32(q, F([[0, 0, 1]]), None, *detail, 4 * CELL, True))
    assert got[2].item() == 72 and got[4][0, 0].item() >= 4 and got[0][0].tolist() == [0, 0, 1]
    assert run(q, F([[0, 0, 1]]), None, detail, 4 * CELL, False, g)[2].item() < 72          # unoriented, the sheet right below wins
    for max_dist, shells in ((8 * CELL, 10), (REACH, 4), (0.0, 2)):                         # rc - s_q > max_dist first holds at r = shells - 1
        got = run(q, F([[1, 0, 0]]), None, detail, max_dist, True, g, debug=True)
        assert got[2].item() == -1 and got[1].item() == float("inf") and got[0][0].tolist() == [1, 0, 0]
        assert got[4][0].tolist() == [shells, 0], got[4]


def test_degenerate_faces_normals_and_queries(lat, queries):
    """Zero-area faces, indices out of range, NaN and inf vertices: not candidates.  NaN, inf and zero vertex normals: the
    fallback.  Zero and NaN query normals: (0, 0, 1).  Invalid and non-finite points: normal 0."""
    v, f, vn = (x.copy() for x in lat)
    q, m, valid, _ = queries
    f[0] = [f[0, 0], f[0, 0], f[0, 1]]                           # zero area
    f[1], f[2], f[80] = [-1, 3, 4], [5, len(v), 6], [7, 8, 2 ** 30]
    v[f[10, 0]], v[f[90, 1]] = F([np.nan, 0, 0]), F([0, np.inf, 0.3])
    vn[f[120, 0]], vn[f[100, 2]] = F([np.nan, 0, 1]), F([0, 0, np.inf])
    vn[f[30]] = 0.0                                              # the interpolated normal of face 30 is 0 everywhere
    centre30 = lat[0][lat[1][30]].mean(0)
    q = np.concatenate([q[:400], [centre30 - F([0, 0, 0.05])]]).astype(F)
    m = np.concatenate([m[:400], F([[0, 0, -4]])])
    valid = np.concatenate([valid[:400], [1]]).astype(np.uint8)
    for oriented in (True, False):
        want = NR.transfer_f32(q, m, valid, v, f, vn, REACH, oriented)
        same(run(q, m, valid, (v, f, vn), REACH, oriented), want)
        assert want[2][-1] == 30 and want[0][-1].tolist() == [0, 0, -1]                     # a hit whose normal is the fallback
        assert not np.isin(want[2], (0, 1, 2, 80)).any() and np.isfinite(want[0]).all()
    assert queries[3][True][0][8].tolist() == [0, 0, 1] and queries[3][True][0][9].tolist() == [0, 0, 1]       # zero and NaN m
    assert queries[3][False][2][8] >= 0                          # ... which still finds a face when orientation is not asked for


def test_empty_inputs(lat, queries):
    v, f, vn = lat
    q, m, valid, _ = queries
    for detail in ((v, f[:0], vn), (v[:0], f[:0], vn[:0]), (v, np.full((5, 3), -1, np.int32), vn)):
        got = run(q[:70], m[:70], valid[:70], detail, REACH, True)
        same(got, NR.transfer_f32(q[:70], m[:70], valid[:70], *detail, REACH, True))
        assert (got[2] == -1).all() and torch.isinf(got[1]).all()
    got = run(q[:0], m[:0], valid[:0], lat, REACH, True)
    assert got[0].shape == (0, 3) and got[2].shape == (0,)


# ---- agreement with the existing query, determinism, the public function


def test_unoriented_equals_closest_on_mesh_bit_for_bit(lat, grid, queries):
    from ngp_pl_amd import mesh
    q, m, valid, _ = queries
    ok = np.ones(len(q), np.uint8)
    for max_dist in (REACH, 8 * CELL, 0.1):
        got = run(q, m, ok, lat, max_dist, False, grid)
        d2, face = mesh.closest_on_mesh(dev(q), to_mesh(*lat), squared=True, max_dist=max_dist, grid=grid)[:2]
        assert torch.equal(got[2], face) and torch.equal(got[1].view(torch.int32), d2.view(torch.int32))


def test_chunks_and_the_public_function(lat, grid, queries):
    from ngp_pl_amd import mesh
    q, m, valid, want = queries
    whole = run(q, m, valid, lat, REACH, True, grid)
    for chunk in (63, 257):
        parts = [run(q[b:b + chunk], m[b:b + chunk], valid[b:b + chunk], lat, REACH, True, grid) for b in range(0, 1000, chunk)]
        for k in range(4):
            assert torch.equal(torch.cat([p[k] for p in parts]).view(torch.int32), whole[k].view(torch.int32))
    d = to_mesh(*lat)
    n, dist, face, bary, dbg = mesh.transfer_normals(dev(q), dev(m), d, REACH, valid=dev(valid), return_debug=True)       # its own grid
    assert np.array_equal(bits(n), bits(want[True][0])) and np.array_equal(face.cpu().numpy(), want[True][2]) and np.array_equal(bits(bary), bits(want[True][3]))
    hit = want[True][2] >= 0
    assert np.allclose(dist.cpu().numpy()[hit], np.sqrt(want[True][1][hit]), rtol=2e-7, atol=0) and np.isinf(dist.cpu().numpy()[~hit]).all()
    assert dbg.shape == (1000, 2) and len(mesh.transfer_normals(dev(q), dev(m), d, REACH, oriented=False, grid=grid)) == 4
    bare = mesh.Mesh(d.vertices, d.faces)                        # without normals of its own: vertex_normals(detail)
    geo = mesh.transfer_normals(dev(q), dev(m), bare, REACH, grid=grid)[0]
    ref = NR.transfer_f32(q, m, None, lat[0], lat[1], mesh.vertex_normals(bare).cpu().numpy(), REACH, True)[0]
    assert np.array_equal(bits(geo), bits(ref))
    for bad in (dict(max_dist=float("inf")), dict(max_dist=-1.0), dict(max_dist=None)):
        with pytest.raises(ValueError, match="max_dist"):
            mesh.transfer_normals(dev(q), dev(m), d, **bad)
    # points beyond (2^14 + 8) cells, whose slack would outgrow a cell, are answered as not valid: no walk at all
    edge = (2.0 ** 14 + 8) * grid.cell
    far = F([[edge, 0, 0], [np.nextafter(F(edge), F(np.inf)), 0, 0], [0, -1e30, 0], [0.1, 0.1, 0.1]])
    n4, d4, f4, _, dbg4 = mesh.transfer_normals(dev(far), dev(np.tile(F([[1, 0, 0]]), (4, 1))), d, REACH, grid=grid, return_debug=True)
    assert f4.tolist() == [-1] * 4 and torch.isinf(d4).all()                              # +x: no face of the sheets is eligible
    assert n4.tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0]]                    # the fallback inside the limit, 0 beyond it
    assert dbg4[1:3].tolist() == [[0, 0], [0, 0]] and 1 <= dbg4[0, 0].item() <= NR.MAX_SHELLS + 2 and dbg4[3, 0].item() == 4
    with pytest.raises(ValueError, match="normals"):
        mesh.transfer_normals(dev(q), dev(m[:5]), d, REACH)


# ---- the shading


def test_shade_against_numpy():
    from ngp_pl_amd import mesh
    g = np.random.RandomState(33)
    C_, H, W = 2, 12, 16
    albedo = g.uniform(0, 1, (C_, H, W, 3)).astype(F)
    samples = g.uniform(0, 1, (C_, H, W, 3)).astype(F)
    ids = g.randint(-1, 50, (C_, H, W)).astype(np.int32)
    ids[0, 0, :4], ids[1, 5, 5] = -1, -7                         # uncovered pixels
    samples[0, 1, 1] = 0.5                                       # 2 s - 1 = 0: no direction
    samples[1, 2, 3] = F([np.nan, 0.5, 0.5])
    ids[0, 1, 1], ids[1, 2, 3] = 4, 5
    lights = np.stack([NR.light_f32((0.3, 0.5, 0.8)), NR.light_f32((-1, 0.2, 0.1))])
    for ambient in (0.0, 0.25, 1.0):
        got = mesh.shade_with_normals(dev(albedo), dev(samples), dev(ids), dev(lights), ambient)
        want = NR.shade_f32(albedo, samples, ids, lights, ambient)
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(got)[ids < 0], bits(albedo)[ids < 0]) and np.array_equal(bits(got[0, 1, 1]), bits(albedo[0, 1, 1]))
        if ambient == 1.0:                                       # k = 1 + 0 * max(...): the frame itself
            assert np.array_equal(bits(got), bits(albedo))
        if ambient == 0.0:
            assert (want[ids >= 0] == 0).all(1).any() and (want[ids >= 0] > 0).any()        # some face away from the light, some towards it
    for bad in (-0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ambient"):
            mesh.shade_with_normals(dev(albedo), dev(samples), dev(ids), dev(lights), bad)
    with pytest.raises(ValueError, match="lights"):
        mesh.shade_with_normals(dev(albedo), dev(samples), dev(ids), dev(lights[:1]), 0.25)


# ---- end to end


@pytest.fixture(scope="module")
def ball():
    """The 24^3 marching-cubes sphere with radial normals (the detail), and its vertex clustering at three voxels."""
    from ngp_pl_amd import mesh
    v, f, n = TR.sphere_mesh(24, radius=0.7, jitter=0.2, seed=4)
    detail = to_mesh(v, f, n)
    low = mesh.simplify_clusters(detail, 3 * 2.0 / 23, origin=(-1, -1, -1))
    assert 50 < low.faces.shape[0] < len(f) / 4
    return (v, f, n), detail, low


BOX = ((-1, -1, -1), (1, 1, 1))


@pytest.mark.parametrize("kind", ["uniform", "adaptive"])
def test_bake_normal_map_equals_the_reference_image(ball, kind):
    from ngp_pl_amd import mesh
    (v, f, n), detail, low = ball
    tex = mesh.texture_atlas(low, texels=2) if kind == "uniform" else mesh.texture_atlas(low, texel_size=0.25, max_texels=4)
    assert isinstance(tex, mesh.Texture if kind == "uniform" else mesh.AdaptiveTexture)
    m = mesh.Mesh(low.vertices, low.faces, low.normals, None, tex)
    max_dist = 4 * 2.0 / 23
    nm = mesh.bake_normal_map(m, detail, max_dist, box=BOX)
    p, d, ok = (x.cpu().numpy() for x in mesh.texel_points(m, tex, BOX))
    image, out = NR.bake_image(p, d, ok, v, f, n, float(F(max_dist)))
    assert nm.image.shape == (tex.height, tex.width, 3) and (nm.width, nm.height) == (tex.width, tex.height)
    assert np.array_equal(nm.image.cpu().numpy().reshape(-1, 3), image)
    assert nm.valid.item() == int(ok.sum()) and nm.hits.item() == int(((out[2] >= 0) & (ok != 0)).sum()) and nm.oriented is True
    assert nm.hits.item() > 0.95 * nm.valid.item() and nm.max_dist == float(F(max_dist))
    for chunk in (1 << 20, 257, 1000):                           # any chunk, and twice: the same bytes
        again = mesh.bake_normal_map(m, detail, max_dist, chunk=chunk, box=BOX)
        assert torch.equal(again.image, nm.image) and again.hits.item() == nm.hits.item()
    loose = mesh.bake_normal_map(m, detail, max_dist)             # the default box: the two meshes' own (only a border texel can be clamped by it)
    assert loose.valid.item() == nm.valid.item() and loose.image.shape == nm.image.shape
    # the map is nearer the sphere's true normals than the clustered mesh's faces are, as on the CPU reference
    live = (ok != 0) & (out[2] >= 0)
    err = NR.angles(NR.decode(image[live]), p[live])
    assert err.mean() < 3.0
    two = mesh.bake_normal_map(m, detail, max_dist, oriented=False, box=BOX)
    assert two.oriented is False and two.hits.item() == nm.hits.item()
    if kind == "uniform":                                        # one brute force more
        assert np.array_equal(two.image.cpu().numpy().reshape(-1, 3), NR.bake_image(p, d, ok, v, f, n, float(F(max_dist)), False)[0])


def test_render_textured_defaults_and_shaded(ball):
    from ngp_pl_amd import mesh
    (v, f, n), detail, low = ball
    colour = lambda p, d: 0.5 + 0.4 * p
    m = mesh.bake_texture(None, low, 2, color_fn=colour, box=BOX)
    nm = mesh.bake_normal_map(m, detail, 4 * 2.0 / 23, box=BOX)
    K, poses, wh = TR.sphere_cameras(2, 32)
    plain = mesh.render_textured(m, K, poses, wh, return_ids=True)
    # the defaults, and either of the two alone, return the unshaded frame bit for bit
    for kw in (dict(normal_map=None, light=None), dict(normal_map=nm), dict(light=(0, 0, 1)), dict(ambient=0.7)):
        got = mesh.render_textured(m, K, poses, wh, return_ids=True, **kw)
        assert all(torch.equal(a, b) if a.dtype == torch.int32 else torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, plain))
    light = (0.3, -0.5, 0.8)
    shaded, ids, depth = mesh.render_textured(m, K, poses, wh, return_ids=True, normal_map=nm, light=light, ambient=0.2)
    assert torch.equal(ids, plain[1]) and torch.equal(depth.view(torch.int32), plain[2].view(torch.int32))
    carrier = mesh.Mesh(m.vertices, m.faces, m.normals, None, mesh.Texture(m.texture.texels, m.texture.width, m.texture.height, m.texture.cells_per_row,
                                                                           m.texture.uvs, nm.image))
    samples = mesh.render_textured(carrier, K, poses, wh)
    lights = np.tile(NR.light_f32(light), (2, 1))
    want = NR.shade_f32(plain[0].cpu().numpy(), samples.cpu().numpy(), ids.cpu().numpy(), lights, 0.2)
    assert np.array_equal(bits(shaded), bits(want)) and not np.array_equal(bits(shaded), bits(plain[0]))
    covered = ids.cpu().numpy() >= 0
    assert covered.any() and not covered.all() and np.array_equal(bits(shaded)[~covered], bits(plain[0])[~covered])
    assert np.array_equal(bits(mesh.render_textured(m, K, poses, wh, normal_map=nm, light=light, ambient=0.2)), bits(want))
    with pytest.raises(ValueError, match="normal_map"):
        mesh.render_textured(m, K, poses, wh, normal_map=object(), light=light)


def test_extract_mesh_and_the_cli(true_density, tmp_path, capsys):
    from ngp_pl_amd import mesh
    from tests.test_meshtex_cpu import read_png
    model = make_model()
    res = 48
    kw = dict(keep_largest=1, simplify_voxels=2)
    plain = mesh.extract_mesh(model, res, texture=dict(texels=4), **kw)
    assert type(plain) is mesh.Mesh                              # without the option: today's class and fields
    got = mesh.extract_mesh(model, res, texture=dict(texels=4, normal_map=True), **kw)
    assert type(got) is mesh.NormalMappedMesh and same_mesh(got, plain) and torch.equal(got.texture.image, plain.texture.image)
    assert torch.equal(got.texture.uvs, plain.texture.uvs)
    nm = got.normal_map
    voxel = 1.0 / (res - 1)
    detail = mesh.extract_mesh(model, res, keep_largest=1)       # the mesh as it stands just before the clustering
    direct = mesh.bake_normal_map(plain, detail, 4.0 * voxel, box=mesh._box(model))
    assert torch.equal(nm.image, direct.image) and nm.hits.item() == direct.hits.item() and nm.max_dist == direct.max_dist and nm.oriented
    share = nm.hits.item() / nm.valid.item()
    assert 0.9 < share <= 1.0
    # the options reach the bake; smoothing comes after it
    other = mesh.extract_mesh(model, res, texture=dict(texels=4, normal_map=dict(max_dist=1.0, oriented=False)), smooth=2, **kw)
    want = mesh.bake_normal_map(plain, detail, 1.0 * voxel, oriented=False, box=mesh._box(model))
    assert torch.equal(other.normal_map.image, want.image) and not other.normal_map.oriented and not torch.equal(other.vertices, plain.vertices)
    assert other.normal_map.hits.item() <= nm.hits.item()
    with pytest.raises(ValueError, match="simplify_voxels or decimate"):
        mesh.extract_mesh(model, res, keep_largest=1, texture=dict(texels=4, normal_map=True))
    dec = mesh.extract_mesh(model, res, keep_largest=1, decimate=300, texture=dict(texel_size=1.0, normal_map=True))
    assert type(dec) is mesh.NormalMappedMesh and isinstance(dec.texture, mesh.AdaptiveTexture) and dec.normal_map.max_dist == float(F(4.0 * voxel))
    assert dec.normal_map.image.shape == (dec.texture.height, dec.texture.width, 3)
    # the CLI
    slim = {"model." + k: x.detach().cpu() for k, x in model.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt = str(tmp_path / "slim.ckpt")
    torch.save(slim, ckpt)
    os.mkdir(str(tmp_path / "a"))
    os.mkdir(str(tmp_path / "b"))
    base = ["--ckpt", ckpt, "--resolution", str(res), "--keep-largest", "1", "--simplify-voxels", "2", "--texture-texels", "4"]
    capsys.readouterr()
    assert mesh.main(base + ["--out", str(tmp_path / "a" / "scene.obj")]) == 0
    first = capsys.readouterr().out.strip().splitlines()
    assert mesh.main(base + ["--texture-normal-map", "--out", str(tmp_path / "b" / "scene.obj")]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(first) == 1 and len(lines) == 2 and lines[0].replace("/b/", "/a/") == first[0]
    record = json.loads(lines[1])["texture_normal_map"]
    assert record == dict(valid_texels=nm.valid.item(), hit_texels=nm.hits.item(), hit_share=share, max_dist=nm.max_dist, oriented=True,
                          width=nm.width, height=nm.height)
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["scene.mtl", "scene.obj", "scene.png"]
    assert set(os.listdir(str(tmp_path / "b"))) == {"scene.mtl", "scene_normal.png", "scene.obj", "scene.png"}
    for name in ("scene.obj", "scene.png"):                      # without the flag nothing changes, with it the other files are the same bytes
        assert open(str(tmp_path / "a" / name), "rb").read() == open(str(tmp_path / "b" / name), "rb").read()
    mtl_a, mtl_b = open(str(tmp_path / "a" / "scene.mtl")).read(), open(str(tmp_path / "b" / "scene.mtl")).read()
    assert mtl_a == "newmtl scene\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd scene.png\n"
    assert mtl_b.startswith(mtl_a) and mtl_b.endswith("norm scene_normal.png\n") and "bump" not in mtl_b.lower()
    assert np.array_equal(read_png(str(tmp_path / "b" / "scene_normal.png")), nm.image.cpu().numpy())
    want_obj = str(tmp_path / "want.obj")
    mesh.save_obj(want_obj, plain)
    assert open(want_obj, "rb").read().replace(b"want", b"scene") == open(str(tmp_path / "a" / "scene.obj"), "rb").read()
    assert mesh.main(base + ["--texture-normal-map", "--texture-normal-max-dist", "1", "--texture-normal-two-sided", "--out", str(tmp_path / "b" / "scene.obj")]) == 0
    two = json.loads(capsys.readouterr().out.strip().splitlines()[-1])["texture_normal_map"]
    assert two["oriented"] is False and two["max_dist"] == float(F(1.0 * voxel)) and two["valid_texels"] == record["valid_texels"]
