"""CPU: the pruned train march's reach table and pre-test (tests/march_prune_reference.py, the numpy restatement of
csrc/march.hip: march_reach_table_kernel, march_reach_far) against the CPU oracle's march, which alone decides: a ray the pre-test
rejects has no oracle sample, and no oracle sample lies at or behind the cut far end.  One cascade, exp_step_factor 0, 128^3."""
import numpy as np
import pytest

from ngp_pl_amd import synthetic as syn
from oracle.vren_oracle import Oracle
from tests import march_prune_reference as P

G, NB = 128, 16
NEAR = 0.01                       # rendering.py:8 NEAR_DISTANCE
MAX_SAMPLES = 1024
CELL = 1.0 / G                    # the box is [-0.5, 0.5]^3


def bitfield_of(cells):
    """128^3 bitfield (Morton order) with the cells of an (n, 3) integer array occupied."""
    grid = np.zeros((1, G ** 3), np.float32)
    if len(cells):
        grid[0, syn.morton3D_np(np.asarray(cells))] = 1.0
    return syn.pack_bitfield_np(grid, 0.5)


def _slab():
    yz = np.stack(np.meshgrid(np.arange(G), np.arange(G), indexing="ij"), -1).reshape(-1, 2)
    return bitfield_of(np.concatenate([np.zeros((len(yz), 1), np.int64), yz], 1))


CASES = {
    # name: (bitfield, sparse: the pre-test must reject some rays and cut some tails)
    "empty": (lambda: bitfield_of(np.zeros((0, 3), np.int64)), True),
    "full": (lambda: np.full(G ** 3 // 8, 255, np.uint8), False),
    "cell_block_corner": (lambda: bitfield_of([[64, 64, 64]]), True),
    "cell_block_face": (lambda: bitfield_of([[72, 67, 67]]), True),
    "cell_grid_border": (lambda: bitfield_of([[127, 60, 0]]), True),
    "cell_grid_corner": (lambda: bitfield_of([[0, 0, 0]]), True),
    "slab_on_box_face": (_slab, True),
    "blob": (lambda: syn.random_blob_bitfield(1, G, 0.08, seed=3), True),
}


def _sphere(g, n, r_lo, r_hi):
    v = g.randn(n, 3)
    return v / np.linalg.norm(v, axis=1, keepdims=True) * g.uniform(r_lo, r_hi, (n, 1))


def rays_for(reach, seed):
    """A few thousand rays: random views of the box, rays aimed within one cell of the dilated region's boundary planes, rays grazing
    box faces and edges, axis-parallel rays; a third of all directions are left un-normalised."""
    import torch
    g = np.random.RandomState(seed)
    o, d = [], []
    # camera-like: origins around the box, aimed at points in and just around it
    n = 1200
    oo = _sphere(g, n, 0.8, 2.0)
    o.append(oo); d.append(g.uniform(-0.6, 0.6, (n, 3)) - oo)
    # the project's own pinhole rays (what training feeds the march)
    K = syn.intrinsics(64)
    dirs = syn.get_ray_directions(64, 64, K)
    poses = syn.hemisphere_poses(4, seed=seed)
    tg = torch.Generator().manual_seed(seed)
    ro, rd = syn.get_rays(dirs[torch.randint(4096, (600,), generator=tg)], poses[torch.randint(4, (600,), generator=tg)])
    o.append(ro.numpy().astype(np.float64)); d.append(rd.numpy().astype(np.float64))
    # aimed at the boundary of the dilated region: points within +-1 cell of a face plane of a reach block that has a clear neighbour
    bz, by, bx = np.nonzero(reach)
    if 0 < len(bx) < NB ** 3:
        blocks = np.stack([bx, by, bz], 1)
        pick = blocks[g.randint(len(blocks), size=1500)]
        axis = g.randint(3, size=1500)
        side = g.randint(2, size=1500)
        p = (pick + g.uniform(0, 1, (1500, 3))) * 8.0                                  # a point of the block, in cells
        p[np.arange(1500), axis] = (pick[np.arange(1500), axis] + side) * 8.0 + g.uniform(-1, 1, 1500)
        target = p * CELL - 0.5
        oo = _sphere(g, 1500, 0.9, 1.8)
        o.append(oo); d.append(target - oo)
    # grazing a box face (parallel to it, within 1e-3 .. 1e-7 of it, either side) and a box edge
    n = 400
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        oo = np.zeros((n, 3)); dd = np.zeros((n, 3))
        off = g.choice([-1, 1], n) * 10.0 ** g.uniform(-7, -3, n)
        oo[:, k] = g.choice([-0.5, 0.5], n) + off
        oo[:, a] = -1.3; oo[:, b] = g.uniform(-0.6, 0.6, n)
        dd[:, a] = 1.0; dd[:, b] = g.uniform(-0.2, 0.2, n); dd[:, k] = g.choice([0.0, 1e-4, -1e-4], n)
        edge = g.rand(n) < 0.3                                                          # ... and along an edge: b pinned next to a face too
        oo[edge, b] = g.choice([-0.5, 0.5], edge.sum()) + off[edge]; dd[edge, b] = 0.0
        o.append(oo); d.append(dd)
    # axis-parallel, through the box and through cell / block boundaries exactly
    n = 300
    for k in range(3):
        oo = (g.randint(0, G + 1, (n, 3)) + g.choice([0.0, 0.5], (n, 1))) * CELL - 0.5
        s = g.choice([-1.0, 1.0], n)
        oo[:, k] = -1.1 * s
        dd = np.zeros((n, 3)); dd[:, k] = s
        o.append(oo); d.append(dd)
    o, d = np.concatenate(o).astype(np.float32), np.concatenate(d)
    norm = np.linalg.norm(d, axis=1, keepdims=True)
    unit = g.rand(len(d), 1) < 0.67
    d = np.where(unit, d / np.maximum(norm, 1e-30), d * 10.0 ** g.uniform(-2, 2, (len(d), 1))).astype(np.float32)
    return o, d


@pytest.fixture(scope="module")
def oracle():
    return Oracle(fma=True)


@pytest.mark.parametrize("name", list(CASES))
def test_pretest_never_removes_an_oracle_sample(oracle, name):
    make, sparse = CASES[name]
    bf = make()
    any_b, reach = P.reach_tables(bf)
    assert any_b.shape == reach.shape == (NB, NB, NB) and not (any_b & ~reach).any()
    assert any_b.any() == reach.any() and reach.sum() >= any_b.sum()
    ro, rd = rays_for(reach, seed=len(name))
    n = len(ro)
    assert 3000 <= n <= 6000
    with np.errstate(all="ignore"):
        _, ht, _ = oracle.ray_aabb_intersect(ro, rd, np.zeros((1, 3), np.float32), np.full((1, 3), 0.5, np.float32), 1)
    hits = ht[:, 0].copy()
    near = (hits[:, 0] >= 0) & (hits[:, 0] < NEAR)
    hits[near, 0] = NEAR                                                                # rendering.py:27-29
    noise = np.random.RandomState(1).rand(n).astype(np.float32)
    rays_a, _, _, _, ts, _ = oracle.raymarching_train(ro, rd, hits, bf, 1, 0.5, 0.0, noise, G, MAX_SAMPLES)
    assert np.array_equal(rays_a[:, 0], np.arange(n))                                   # the oracle packs in ray order
    count = rays_a[:, 2]
    rejected, t2_cut, tested = P.pretest(ro, rd, hits[:, 0], hits[:, 1], reach)
    assert (t2_cut <= hits[:, 1])[hits[:, 0] >= 0].all()
    assert not (rejected & (count > 0)).any(), "rejected rays with oracle samples: %s" % np.nonzero(rejected & (count > 0))[0][:8]
    ray_of = np.repeat(np.arange(n), count)
    behind = ts >= t2_cut[ray_of]
    assert not behind.any(), "oracle samples at or behind the cut far end, rays %s" % np.unique(ray_of[behind])[:8]
    hit = hits[:, 0] >= 0
    share = rejected.sum() / max(hit.sum(), 1)
    cut = (tested & ~rejected & (t2_cut < hits[:, 1])).sum()
    print("%s: %d rays, %d hit the box, %d tested, rejected share %.3f, tails cut %d, oracle samples %d"
          % (name, n, hit.sum(), tested.sum(), share, cut, len(ts)))
    assert tested.sum() > 0.9 * hit.sum()                                               # the pre-test runs on (nearly) every hit
    if sparse:
        assert rejected.sum() > 0, "a sparse grid and nothing rejected: the test would pass by pruning nothing"
        if any_b.any():
            assert cut > 0 and (count[tested & ~rejected] > 0).any()
    if name == "empty":
        assert rejected[tested].all() and len(ts) == 0


def test_reach_table_is_the_dilation_of_any():
    """The table by definition on a grid small enough to state directly: reach = any dilated by one block, clamped at the border."""
    bf = bitfield_of([[64, 64, 64], [127, 60, 0]])
    any_b, reach = P.reach_tables(bf)
    assert any_b.sum() == 2 and any_b[8, 8, 8] and any_b[0, 7, 15]
    want = np.zeros((NB, NB, NB), bool)
    want[7:10, 7:10, 7:10] = True                      # block (8, 8, 8), indexed [bz, by, bx]
    want[0:2, 6:9, 14:16] = True                       # block (15, 7, 0)
    assert np.array_equal(reach, want)
