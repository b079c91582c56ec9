"""GPU: libngp_meshdist.so against the numpy restatement (tests/mesh_distance_reference.py), as integer words: the sampler's points,
weights, face ids and totals; the query's squared distances, faces and closest points against the brute-force minimum, for queries
placed on cell faces, edges and corners, outside the grid, on the early-exit boundary and on ties, and for every grid the same
words; the statistics within the f64 bound of exactly rounded sums; known answers through mesh_distance; the vertex-clustering
bound across libraries; the export against the procedural scene's true surface; and the CLI."""
import json
import math

import numpy as np
import pytest
import torch

from tests import mc_reference as MC
from tests import mesh_distance_reference as R

pytestmark = pytest.mark.gpu
F = np.float32


def words(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def to_mesh(v, f, device="cuda"):
    from ngp_pl_amd import mesh
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return mesh.Mesh(t(np.asarray(v, F).reshape(-1, 3)), t(np.asarray(f, np.int32).reshape(-1, 3)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the sampler


def _sampler_mesh(n_faces, seed):
    """Random triangles whose longest edges give k = 1, 2, 3 at spacing 1, then (from 8 faces on) two faces with k = 64, one whose
    edge would give k > 64, and faces that are skipped: an index -1, an index n_vertices, a NaN vertex."""
    g = np.random.RandomState(seed)
    v = g.uniform(-1, 1, (3 * n_faces, 3))
    f = np.arange(3 * n_faces).reshape(-1, 3)
    for face in range(n_faces):
        a = v[3 * face]
        e1, e2 = g.normal(size=3), g.normal(size=3)
        e1, e2 = e1 / np.linalg.norm(e1), e2 / np.linalg.norm(e2)
        length = (0.7, 1.6, 2.5)[face % 3]
        v[3 * face + 1], v[3 * face + 2] = a + length * e1, a + 0.6 * length * e2
    v = v.astype(F)
    f = f.astype(np.int32)
    if n_faces >= 8:
        v[3 * 1 + 1] = v[3 * 1] + F(63.5) * np.array([1, 0, 0], F)
        v[3 * 1 + 2] = v[3 * 1] + np.array([0, 1, 0], F)
        v[3 * 4 + 1] = v[3 * 4] + F(64.0) * np.array([0, 1, 0], F)            # exactly 64 spacings: k = 64 unclamped
        v[3 * 4 + 2] = v[3 * 4] + np.array([0, 0, 1], F)
        v[3 * 5 + 1] = v[3 * 5] + F(1000.0) * np.array([0, 0, 1], F)          # k would be 1001
        f[2, 0], f[3, 2], v[3 * 6 + 1, 1] = -1, 3 * n_faces, np.nan
        f[n_faces - 1, 1] = -7
    return v, f


@pytest.mark.parametrize("n_faces", [1, 63, 64, 65, 255, 256, 257, 2049])
def test_sampler_points_weights_ids_and_totals_are_exact(n_faces):
    from ngp_pl_amd import _meshdist_lib as L, mesh
    assert L.SCAN_BLOCK == 2048
    v, f = _sampler_mesh(n_faces, n_faces)
    pts, wts, ids, counts = R.sample_f32(v, f, 1.0)
    if n_faces >= 8:
        assert counts[[1, 4, 5]].tolist() == [4096] * 3 and counts[[2, 3, 6, n_faces - 1]].tolist() == [0] * 4
        assert {1, 4, 9} <= set(counts.tolist())
    m = to_mesh(v, f)
    got = mesh.sample_surface(m, 1.0)
    again = mesh.sample_surface(m, 1.0)
    assert got[0].shape[0] == int(counts.sum()) == len(pts)
    assert np.array_equal(words(got[0]), words(pts)) and np.array_equal(words(got[1]), words(wts))
    assert np.array_equal(got[2].cpu().numpy(), ids)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, again))


def test_sampler_of_nothing():
    from ngp_pl_amd import mesh
    v, f = _sampler_mesh(4, 0)
    for m in (to_mesh(v, f[:0]), to_mesh(v[:0], f[:0]), to_mesh(v, np.full((5, 3), -1))):
        p, w, i = mesh.sample_surface(m, 0.5)
        assert p.shape == (0, 3) and w.shape == (0,) and i.shape == (0,)


# ---- the query

SQUARE_Z = 2.0


@pytest.fixture(scope="module")
def target():
    """A marching-cubes sphere at 24^3, three dozen random large triangles that span many cells, a unit square in the plane
    z = 2 cut along its diagonal (faces that share an edge and two vertices), and that square's first triangle once more (a
    bit-equal tie)."""
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, 24, dtype=F)] * 3, indexing="ij")
    v, f, _, _ = MC.marching_cubes((F(0.7) - np.sqrt(x * x + y * y + z * z)).astype(F), 0.0, (-1, -1, -1), (1, 1, 1))
    g = np.random.RandomState(11)
    big = g.uniform(-1.5, 1.5, (36, 3, 3)).astype(F)
    sq = np.array([[0, 0, SQUARE_Z], [1, 0, SQUARE_Z], [1, 1, SQUARE_Z], [0, 1, SQUARE_Z]], F)
    n0 = len(v)
    v = np.concatenate([v.astype(F), big.reshape(-1, 3), sq])
    n1 = n0 + 108
    f = np.concatenate([f.astype(np.int32), n0 + np.arange(108, dtype=np.int32).reshape(-1, 3),
                        np.array([[n1, n1 + 1, n1 + 2], [n1, n1 + 2, n1 + 3], [n1, n1 + 1, n1 + 2]], np.int32)])
    return v, f


def _refine(p, direction, want, v, f):
    """p moved along direction until the rule's own distance to the nearest face is `want` as closely as f32 allows."""
    p = p.astype(np.float64)
    for _ in range(4):
        d = math.sqrt(float(R.query_f32(p.astype(F)[None], v, f)[0][0]))
        p = p + direction * (want - d)
    return p.astype(F)


@pytest.fixture(scope="module")
def queries(target):
    from ngp_pl_amd import mesh
    v, f = target
    grid = mesh.distance_grid(to_mesh(v, f))
    o, cell, dims = np.array(grid.origin, F), F(grid.cell), grid.dims
    g = np.random.RandomState(12)
    lo, hi = o, o + np.array(dims, F) * cell
    q = [g.uniform(lo, hi, (150, 3))]                                            # inside cells
    corner = lambda i, j, k: o + np.array([i, j, k], F) * cell
    for _ in range(20):                                                          # on cell faces, edges and corners
        i, j, k = (g.randint(0, n + 1) for n in dims)
        h = g.uniform(0, 1, 3).astype(F) * cell
        q += [corner(i, j, k)[None], (corner(i, j, k) + h * np.array([0, 1, 1], F))[None], (corner(i, j, k) + h * np.array([0, 0, 1], F))[None],
              (corner(i, j, k) + h * np.array([1, 0, 1], F))[None]]
    ext = hi - lo
    for axis in range(3):                                                        # beyond each of the 6 sides, beyond corners
        for side in (-1, 1):
            p = g.uniform(lo, hi, (4, 3))
            p[:, axis] = (lo[axis] - g.uniform(0.01, 2, 4) * ext[axis]) if side < 0 else (hi[axis] + g.uniform(0.01, 2, 4) * ext[axis])
            q.append(p)
    q += [(hi + 0.3 * ext)[None], (lo - 1.7 * ext)[None], np.array([[hi[0] + 1, lo[1] - 1, hi[2] + 2]]), (hi + 40 * ext)[None]]
    for r in (1, 2, 3):                                                          # the early-exit boundary r * cell
        for direction in (np.array([1.0, 0, 0]), np.array([0.48, -0.6, 0.64]), np.array([0, 0, -1.0])):
            want = float(F(r) * cell)
            base = _refine(direction * (0.7 + want), direction, want, v, f)
            ulp = float(np.spacing(np.abs(base).max()))
            s = float(R.slack(max(np.abs(base).max(), np.abs(lo).max(), np.abs(hi).max())))
            for step in (-3 * ulp, -2 * ulp, -ulp, 0.0, ulp, 2 * ulp, 3 * ulp, -s, s, -s - ulp, s + ulp):
                q.append((base.astype(np.float64) + direction * step)[None])
            inner = _refine(direction * (0.7 - want), -direction, want, v, f)   # the same from inside the sphere
            q += [inner[None], (inner.astype(np.float64) + direction * ulp)[None], (inner.astype(np.float64) - direction * s)[None]]
        top = float(F(SQUARE_Z) + F(r) * cell)                                 # and straight over the square, where the distance is exact
        ulp, s = float(np.spacing(F(top))), float(R.slack(max(top, np.abs(lo).max(), np.abs(hi).max())))
        q.append(np.array([[0.3, 0.6, top + step] for step in (-2 * ulp, -ulp, 0.0, ulp, 2 * ulp, -s, s)]))
    q.append(np.zeros((3, 3)) + g.uniform(-0.02, 0.02, (3, 3)))                  # the centre: several empty shells
    # ties: over the shared diagonal and over the shared vertices of the square, at several heights, and over the doubled face
    for h in (0.25, 0.5, 1.0, -0.125):
        q.append(np.array([[0.5, 0.5, SQUARE_Z + h], [0.25, 0.25, SQUARE_Z + h], [0.75, 0.75, SQUARE_Z + h], [0, 0, SQUARE_Z + h], [1, 1, SQUARE_Z + h],
                           [-0.5, -0.5, SQUARE_Z + h], [1.5, 1.25, SQUARE_Z + h], [0.75, 0.25, SQUARE_Z + h], [0.25, 0.75, SQUARE_Z + h]]))
    q.append(np.array([[np.nan, 0, 0], [0, np.inf, 0], [0.1, 0.2, -np.inf]]))
    q = np.concatenate([np.asarray(x, np.float64).reshape(-1, 3) for x in q]).astype(F)
    return q, R.query_f32(q, v, f), grid


def _run(q, v, f, grid=None, **kw):
    from ngp_pl_amd import mesh
    return mesh.closest_on_mesh(dev(q), to_mesh(v, f), squared=True, return_points=True, grid=grid, **kw)


def _same(got, want):
    d2, face, q = got[:3]
    assert np.array_equal(words(d2), words(want[0])), int((words(d2) != words(want[0])).sum())
    assert np.array_equal(face.cpu().numpy(), want[1])
    assert np.array_equal(words(q), words(want[2]))


def test_query_words_equal_the_brute_force_minimum(target, queries):
    v, f = target
    q, want, grid = queries
    assert (want[1] >= 0).sum() == len(q) - 3 and want[1][-3:].tolist() == [-1] * 3
    tie = want[1] == len(f) - 3                                # the doubled face never wins over its first copy
    assert tie.sum() >= 8 and not (want[1] == len(f) - 1).any()
    got = _run(q, v, f, grid=grid, return_debug=True)
    _same(got, want)
    shells = got[3][:, 0].cpu().numpy()
    assert shells[:-3].min() >= 1 and shells.max() >= 4 and not shells[-3:].any()     # several shells where the surroundings are empty
    _same(_run(q, v, f, grid=grid), want)                      # two runs, the same bits


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_query_counts_around_the_wave_and_the_workgroup(target, queries, n):
    v, f = target
    q, want, grid = queries
    pick = np.random.RandomState(n).permutation(len(q))[:n]
    _same(_run(q[pick], v, f, grid=grid), tuple(w[pick] for w in want))


def test_every_grid_gives_the_same_words(target, queries):
    from ngp_pl_amd import mesh
    v, f = target
    q, want, _ = queries
    m = to_mesh(v, f)
    lo, ext = v.min(0), v.max(0) - v.min(0)
    grids = [mesh.distance_grid(m, cell=float(ext.max()) * 1.01, origin=lo - 0.005 * ext, dims=(1, 1, 1)),
             mesh.distance_grid(m, cell=float(ext.max()) / 1.9, origin=lo - 0.01 * ext, dims=(2, 3, 5)),
             mesh.distance_grid(m, cell=float(ext.max()) / 9, origin=lo + 0.2 * ext, dims=(2, 3, 5)),      # covers a corner of the target only
             mesh.distance_grid(m, cell=0.31)]
    # 128, 256 and 258 blocks of 2048 cells for the one-workgroup scan of the block sums: 256 is where its earlier form began a
    # second chunk.  The target lies inside the first 64 cells along x, so the cells added along x are empty: the same entries.
    fine = [mesh.distance_grid(m, cell=float(ext.max()) * 1.01 / 64, origin=lo - 0.005 * ext, dims=d) for d in ((64, 64, 64), (128, 64, 64), (129, 64, 64))]
    assert fine[2].dims == (129, 64, 64) and fine[0].n_entries == fine[1].n_entries == fine[2].n_entries > grids[0].n_entries
    assert grids[0].dims == (1, 1, 1) and grids[1].dims == (2, 3, 5) and grids[0].n_entries == int(R.usable(v, f).sum())
    for grid in grids:
        _same(_run(q, v, f, grid=grid), want)
    near = ((q >= lo) & (q <= lo + ext)).all(1)                # a query far outside walks every shell of half a million cells
    assert near.sum() >= 150
    for grid in fine:
        _same(_run(q[near], v, f, grid=grid), tuple(w[near] for w in want))


def test_permuted_faces_agree_after_mapping_back(target, queries):
    v, f = target
    q, want, _ = queries
    perm = np.random.RandomState(13).permutation(len(f))       # new face j is old face perm[j]
    new_of = np.argsort(perm)
    first, copy = new_of[len(f) - 3], new_of[len(f) - 1]
    if first < copy:                                           # the doubled face's second copy comes first now
        perm[[first, copy]] = perm[[copy, first]]
    fp = f[perm]
    got = _run(q, v, fp)
    expect = R.query_f32(q, v, fp)                             # what it must be: a bit-equal tie goes to the smaller NEW index
    _same(got, expect)
    assert np.array_equal(words(got[0]), words(want[0]))       # the distance does not depend on the order
    face = got[1].cpu().numpy()
    back = np.where(face >= 0, perm[np.clip(face, 0, None)], -1)
    assert ((back == len(f) - 1) & (want[1] == len(f) - 3)).sum() >= 8 and not (back == len(f) - 3).any()


def test_max_dist_below_at_and_above(target, queries):
    v, f = target
    q = np.array([[0.25, 0.5, SQUARE_Z + 0.25], [0.75, 0.5, SQUARE_Z + 0.25], [0.5, 0.125, SQUARE_Z - 0.25]], F)
    full = R.query_f32(q, v, f)
    assert full[0].tolist() == [0.0625] * 3                    # exactly a quarter from the square
    for max_dist, hit in ((float(np.nextafter(F(0.25), F(0))), False), (0.25, True), (float(np.nextafter(F(0.25), F(1))), True), (0.0, False)):
        got = _run(q, v, f, max_dist=max_dist)
        _same(got, R.query_f32(q, v, f, max_dist))
        assert (got[1].cpu().numpy() >= 0).tolist() == [hit] * 3
        assert bool(torch.isinf(got[0]).all()) == (not hit) and bool(torch.isnan(got[2]).all()) == (not hit)
    allq, want, grid = queries
    for max_dist in (0.05, 0.3):
        _same(_run(allq, v, f, grid=grid, max_dist=max_dist), R.query_f32(allq, v, f, max_dist))
    on = np.array([[0.5, 0.25, SQUARE_Z]], F)                  # on the face: max_dist = 0 is a hit
    assert _run(on, v, f, max_dist=0.0)[1].tolist() == R.query_f32(on, v, f, 0.0)[1].tolist() and R.query_f32(on, v, f, 0.0)[1][0] >= 0


def test_targets_without_a_usable_face_give_all_misses(target, queries):
    v, f = target
    q = queries[0][:70]
    bad = f[:40].copy()
    bad[::2, 0], bad[1::2, 2] = -1, len(v)
    vn = v.copy()
    vn[f[:5].ravel()] = np.nan
    for vv, ff in ((v, f[:0]), (v[:0], f[:0]), (v, bad), (vn, f[:5])):
        got = _run(q, vv, ff)
        assert (got[1] == -1).all() and torch.isinf(got[0]).all() and torch.isnan(got[2]).all()
        _same(got, R.query_f32(q, vv, ff))


def test_distances_and_points_of_the_python_surface(target, queries):
    from ngp_pl_amd import mesh
    v, f = target
    q, want, grid = queries
    d, face = mesh.closest_on_mesh(dev(q), to_mesh(v, f))
    assert torch.equal(face.cpu(), torch.from_numpy(want[1]))
    hit = want[1] >= 0
    assert np.allclose(d.cpu().numpy()[hit], np.sqrt(want[0][hit]), rtol=2e-7, atol=0) and np.isinf(d.cpu().numpy()[~hit]).all()
    with pytest.raises(ValueError):
        mesh.closest_on_mesh(dev(q), to_mesh(v, f), max_dist=-1.0)
    with pytest.raises(ValueError):
        mesh.closest_on_mesh(dev(q).double(), to_mesh(v, f))


# ---- the statistics


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 131072, 131073])
def test_statistics_within_the_f64_bound_and_bit_identical(n):
    from ngp_pl_amd import _meshdist_lib as L, mesh
    assert L.STATS_MAX_BLOCKS * 256 == 131072                  # the stride of the largest launch
    g = np.random.RandomState(n)
    d2 = (g.uniform(0, 2, n) ** 2).astype(F)
    face = g.randint(0, 1000, n).astype(np.int32)
    miss = g.rand(n) < 0.2
    if n > 1:
        miss[0], miss[-1] = False, True
    face[miss] = -1
    d2[miss] = np.inf
    w = g.uniform(0, 3, n).astype(F)
    th = (0.5, 1.0, 1.5, 0.0, 3.0)
    want, mag = R.stats_fsum(d2, face, w, th)
    got = mesh.distance_statistics(dev(d2), dev(face), dev(w), th)
    again = mesh.distance_statistics(dev(d2), dev(face), dev(w), th)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))
    got = got.cpu().tolist()
    for k in range(14):
        if k in (3, 5):
            assert got[k] == want[k], k                        # the maximum and the number of misses: exact
        else:
            assert abs(got[k] - want[k]) <= n * 2.0 ** -53 * mag[k], (k, got[k], want[k])
    # with unit weights the sums within the thresholds are counts: exact
    ones = np.ones(n, F)
    got = mesh.distance_statistics(dev(d2), dev(face), dev(ones), th).cpu().tolist()
    hit = ~miss
    assert got[0] == hit.sum() and got[4] == got[5] == miss.sum()
    assert got[6:11] == [int((hit & (d2 <= F(t) * F(t))).sum()) for t in th] and got[11:] == [0.0] * 3
    assert mesh.distance_statistics(dev(d2), dev(face), dev(ones)).cpu().tolist()[6:] == [0.0] * 8


# ---- known answers through the Python surface


def _square(n, step, z):
    xs = np.arange(n + 1) * step
    v = np.array([[x, y, z] for y in xs for x in xs], F)
    f = []
    for j in range(n):
        for i in range(n):
            a = j * (n + 1) + i
            b, c, d = a + 1, a + n + 1, a + n + 2
            f += [[a, b, d], [a, d, c]] if (i + j) % 2 == 0 else [[a, b, c], [b, d, c]]
    return v, np.array(f, np.int32)


def test_two_parallel_squares_a_quarter_apart():
    from ngp_pl_amd import mesh
    a, b = to_mesh(*_square(8, 0.25, 0.0)), to_mesh(*_square(2, 1.0, 0.25))       # the square [0, 2]^2, 128 and 8 faces
    for spacing in (0.5, 0.2, None):
        r = mesh.mesh_distance(a, b, spacing=spacing, thresholds=(0.25, 0.125), per_vertex=True)
        for side in ("a_to_b", "b_to_a"):
            s = r[side]
            assert s["mean"] == s["rms"] == s["max"] == 0.25 and s["miss_share"] == 0.0 and s["within"] == [1.0, 0.0]
            assert abs(s["area"] - 4.0) < 1e-6                   # f32 areas, k * k-th parts of 1/32 and 1/2
        assert r["chamfer"] == 0.5 and r["hausdorff"] == 0.25 and r["fscore"] == [1.0, 0.0]
        assert r["precision"] == [1.0, 0.0] and r["recall"] == [1.0, 0.0] and r["thresholds"] == [0.25, 0.125]
        assert (r["vertex_distance"] == 0.25).all() and r["vertex_distance"].shape == (81,)
        for src, dst in ((a, b), (b, a)):                        # every sample, and the unweighted mean
            p, w, _ = mesh.sample_surface(src, r["spacing"])
            d, face = mesh.closest_on_mesh(p, dst)
            assert (mesh.closest_on_mesh(p, dst, squared=True)[0] == 0.0625).all()
            assert (d == 0.25).all() and (face >= 0).all() and p.shape[0] == r["a_to_b" if src is a else "b_to_a"]["samples"]
            st = mesh.distance_statistics(d * d, face, torch.ones_like(w)).tolist()
            assert st[1] / st[0] == 0.25 and st[0] == p.shape[0]
    r = mesh.mesh_distance(a, b, spacing=0.5, thresholds=(0.25,), max_dist=0.125)   # nothing within reach: all area missed
    assert r["a_to_b"]["miss_share"] == 1.0 and r["b_to_a"]["miss_share"] == 1.0 and r["fscore"] == [0.0] and math.isnan(r["chamfer"])


def test_a_mesh_against_itself_is_at_distance_zero(target):
    """Vertices sit in a vertex case of the rule: q is the vertex itself, for any mesh.  A centroid's closest point is computed
    through the interior case and equals the centroid only where those products and quotients are exact, as on these lattice
    squares; on a general mesh it is within the header's E of it."""
    from ngp_pl_amd import mesh
    for n, step in ((4, 0.75), (8, 0.375), (2, 1.5)):
        m = to_mesh(*_square(n, step, 0.0))
        for spacing in (2.0, 0.6):
            r = mesh.mesh_distance(m, m, spacing=spacing, thresholds=(0.0,), per_vertex=True)
            assert r["chamfer"] == 0.0 and r["hausdorff"] == 0.0 and r["fscore"] == [1.0] and not r["vertex_distance"].any()
            p, _, _ = mesh.sample_surface(m, spacing)
            assert not mesh.closest_on_mesh(p, m, squared=True)[0].any()
    v, f = target
    m = to_mesh(v, f)
    assert not mesh.closest_on_mesh(m.vertices, m, squared=True)[0].any()
    r = mesh.mesh_distance(m, m)
    assert r["a_to_b"] == r["b_to_a"] and r["a_to_b"]["miss_share"] == 0


# ---- across libraries, and against the truth


def _scene(res, fn):
    from ngp_pl_amd import mesh
    lo, hi = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
    xyz = mesh.lattice_points((res,) * 3, (lo, hi))
    return fn(xyz).view(res, res, res).contiguous(), (lo, hi), 1.0 / (res - 1)


def test_clustered_vertices_stay_within_the_cell_diagonal_of_the_original():
    from ngp_pl_amd import mesh, synthetic as syn
    vol, bounds, voxel = _scene(64, syn.density)
    original = mesh.marching_cubes(vol, syn.SIGMA_INSIDE / 2, bounds)
    grid = mesh.distance_grid(original)
    for voxels in (2, 4):
        cell = voxels * voxel
        slim = mesh.simplify_clusters(original, cell, origin=bounds[0])
        assert 0 < slim.vertices.shape[0] < original.vertices.shape[0] / 2
        d, face = mesh.closest_on_mesh(slim.vertices, original, grid=grid)
        assert (face >= 0).all() and float(d.max()) <= math.sqrt(3.0) * cell, (voxels, float(d.max()), cell)
        assert float(d.max()) > 0


def test_export_against_the_true_surface_is_within_a_lattice_diagonal():
    from ngp_pl_amd import mesh, synthetic as syn
    vol, bounds, voxel = _scene(64, syn.density)
    export = mesh.marching_cubes(vol, syn.SIGMA_INSIDE / 2, bounds)
    sd, _, _ = _scene(64, lambda x: -syn.signed_distance(x))
    truth = mesh.marching_cubes(sd, 0.0, bounds)
    r = mesh.mesh_distance(export, truth, thresholds=(voxel, voxel / 4))
    print("64^3 export against the level-0 mesh of the signed distance:", json.dumps(r))
    assert 0 < r["hausdorff"] < math.sqrt(3.0) * voxel
    assert r["a_to_b"]["miss_share"] == 0 and r["b_to_a"]["miss_share"] == 0 and 0 < r["chamfer"] <= 2 * r["hausdorff"]


# ---- the CLI


def test_cli_distance_to(monkeypatch, tmp_path, capsys):
    from ngp_pl_amd import mesh, synthetic as syn
    from ngp_pl_amd.networks import NGP

    def volume(model, resolution=512, bounds=None, chunk=0):
        nx, ny, nz = mesh._resolution(resolution)
        return syn.density(mesh.lattice_points((nx, ny, nz), mesh._bounds(model, bounds))).view(nz, ny, nx).contiguous()

    monkeypatch.setattr(mesh, "density_volume", volume)
    torch.manual_seed(3)
    model = NGP(scale=0.5).cuda()
    model.register_training_buffers()
    slim = {"model." + k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt, ref, out, plain, rec = (str(tmp_path / n) for n in ("slim.ckpt", "ref.ply", "out.ply", "plain.ply", "rec.json"))
    torch.save(slim, ckpt)
    base = ["--ckpt", ckpt, "--resolution", "32", "--threshold", str(syn.SIGMA_INSIDE / 2)]
    assert mesh.main(base + ["--out", ref]) == 0
    first = capsys.readouterr().out.strip().splitlines()
    assert mesh.main(base + ["--simplify-voxels", "2", "--out", plain]) == 0
    capsys.readouterr()
    assert mesh.main(base + ["--simplify-voxels", "2", "--out", out, "--distance-to", ref, "--distance-thresholds", "0.03,0.06",
                             "--distance-out", rec]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and len(first) == 1 and lines[0].replace(out, plain).startswith(plain)
    record = json.loads(lines[1])
    assert json.loads(open(rec).read()) == record
    assert set(record) == {"a_to_b", "b_to_a", "chamfer", "hausdorff", "thresholds", "precision", "recall", "fscore", "spacing"}
    for side in ("a_to_b", "b_to_a"):
        assert set(record[side]) == {"area", "samples", "mean", "rms", "max", "miss_share", "within"}
    assert 0 < record["hausdorff"] < 1 and record["chamfer"] > 0 and len(record["fscore"]) == 2
    # the export itself does not change with the flag, and is what the library call gives
    assert open(out, "rb").read() == open(plain, "rb").read()
    want = str(tmp_path / "want.ply")
    mesh.save_ply(want, mesh.extract_mesh(model, 32, threshold=syn.SIGMA_INSIDE / 2, simplify_voxels=2))
    assert open(want, "rb").read() == open(plain, "rb").read()
    for bad in (["--distance-spacing", "0.1"], ["--distance-to", ref, "--distance-spacing", "0"], ["--distance-to", ref, "--distance-thresholds", "a"]):
        with pytest.raises(SystemExit):
            mesh.main(base + ["--out", out] + bad)
