"""The numpy restatement of the occupancy update (tests/occupancy_reference.py) against the reference project's own statement of
it, its random stream's uniformity at fixed seeds, and the conditions that the inputs of tests/test_occupancy_exact_gpu.py must meet
-- all without a GPU."""
import numpy as np
import pytest
import torch

from tests import occupancy_reference as R


def random_half(G, seed=0):
    return R.pattern_grid("random_half", 1, G, R.THR, seed, R.GRID_LO, R.GRID_HI)[0]


@pytest.mark.parametrize("G", [4, 64])
@pytest.mark.parametrize("warmup", [False, True])
def test_positions_are_the_reference_projects_float32_expression(G, warmup):
    """networks.py:253-255 in torch float32, fed the stream's `rand`, for all six cascades: within position_bound of the float64
    positions (torch rounds both products and the sum, one of the evaluation orders the bound allows), and every position within
    half a cell of its cell's centre."""
    grid = random_half(G)
    worst = 0.0
    for c in range(R.CASCADES):
        d = R.draws(3, c, G, R.SCALE, grid, R.THR, warmup)
        assert d.pos.shape == ((G ** 3 if warmup else G ** 3 // 2), 3)
        coords, rand = torch.from_numpy(d.coords), torch.from_numpy(d.u)
        assert coords.dtype == torch.int32 and rand.dtype == torch.float32
        s = min(2 ** (c - 1), R.SCALE)
        half_grid_size = s / G
        xyzs_w = (coords / (G - 1) * 2 - 1) * (s - half_grid_size)
        xyzs_w += (rand * 2 - 1) * half_grid_size
        assert xyzs_w.dtype == torch.float32
        bound = R.position_bound(c, G, R.SCALE)
        err = np.abs(xyzs_w.numpy().astype(np.float64) - d.pos).max()
        worst = max(worst, err / bound)
        assert err <= bound, (c, err, bound)
        centre = (d.coords.astype(np.float64) / (G - 1) * 2 - 1) * (s - half_grid_size)
        off = np.abs(d.pos - centre)
        assert off.max() <= half_grid_size + bound, (c, off.max() / half_grid_size)      # A, f32(s - hgs), f32(hgs): one rounding below s each
        assert off.max() > 0.9 * half_grid_size
        assert (d.u >= 0).all() and (d.u < 1).all()
    print("torch float32 positions: worst error / bound = %.3f" % worst)


def test_cells_are_the_reference_projects_draws():
    """Uniform half: the coordinates' Morton index, in range.  Occupied half: networks.py:186-192 with the stream's `rand` -- restated
    a second way here, as the product's torch path has it (cumsum + searchsorted) --, always an occupied cell; an empty set maps every
    draw to the last cell; warm-up is every cell once in order."""
    for G in (4, 16, 32):
        grid = random_half(G, seed=G)
        cells_n, M = G ** 3, G ** 3 // 4
        d = R.draws(11, 2, G, R.SCALE, grid, R.THR, False)
        assert d.cells.shape == (2 * M,) and d.M == M
        x, y, z = (d.coords[:, k].astype(np.int64) for k in range(3))
        assert d.coords.min() >= 0 and d.coords.max() < G
        plain = np.zeros(2 * M, np.int64)
        for b in range(8):
            plain |= ((x >> b) & 1) << (3 * b) | ((y >> b) & 1) << (3 * b + 1) | ((z >> b) & 1) << (3 * b + 2)
        assert np.array_equal(plain, d.cells)
        occ = grid > np.float32(R.THR)
        assert occ[d.cells[M:]].all()
        u = R.u01(R.occ_hash(R.stream_base(11, 2, np.arange(M, 2 * M)) + np.uint64(3)))
        csum = torch.cumsum(torch.from_numpy(occ), 0, dtype=torch.int32)
        rank = (torch.from_numpy(u) * csum[-1]).to(torch.int32)
        want = torch.searchsorted(csum, rank, right=True).clamp_(max=cells_n - 1)
        assert np.array_equal(want.numpy(), d.cells[M:])
        empty = R.draws(11, 2, G, R.SCALE, np.minimum(grid, np.float32(R.THR)), R.THR, False)
        assert (empty.cells[M:] == cells_n - 1).all() and np.array_equal(empty.cells[:M], d.cells[:M])
        w = R.draws(11, 2, G, R.SCALE, grid, R.THR, True)
        assert np.array_equal(w.cells, np.arange(cells_n)) and w.M == 0


def chi2(counts, expect):
    return float(((counts - expect) ** 2 / expect).sum())


@pytest.mark.parametrize("G", [32, 64])
@pytest.mark.parametrize("c", [0, 5])
@pytest.mark.parametrize("seed", [1, 2, 1000004])
def test_the_stream_is_uniform_at_fixed_seeds(G, c, seed):
    """chi^2 < df + 5 sqrt(2 df): the uniform half over 8^3 blocks of cells and per axis, the occupied half's ranks over 512 slices of
    the occupied set."""
    grid = random_half(G, seed=9)
    d = R.draws(seed, c, G, R.SCALE, grid, R.THR, False)
    M = d.M
    def limit(df):
        return df + 5 * (2 * df) ** 0.5
    blk = d.coords[:M] // (G // 8)
    counts = np.bincount(blk[:, 0] + 8 * blk[:, 1] + 64 * blk[:, 2], minlength=512)
    x_blocks = chi2(counts, M / 512)
    assert x_blocks < limit(511), x_blocks
    x_axis = max(chi2(np.bincount(d.coords[:M, k], minlength=G), M / G) for k in range(3))
    assert x_axis < limit(G - 1), x_axis
    occ = np.flatnonzero(grid > np.float32(R.THR))
    rank = np.searchsorted(occ, d.cells[M:])
    assert np.array_equal(occ[rank], d.cells[M:])
    x_occ = chi2(np.bincount(rank * 512 // len(occ), minlength=512), M / 512)     # slices differ by at most one cell in len(occ) / 512 >= 32
    assert x_occ < limit(511), x_occ
    print("G %d cascade %d seed %d: chi2 blocks %.0f (< %.0f), axis %.0f (< %.0f), occupied %.0f" % (G, c, seed, x_blocks, limit(511), x_axis, limit(G - 1), x_occ))


def test_cascades_and_consecutive_seeds_draw_different_cells():
    for G in (32, 64):
        grid = random_half(G)
        M = G ** 3 // 4
        a = R.draws(5, 0, G, R.SCALE, grid, R.THR, False)
        for other in (R.draws(5, 1, G, R.SCALE, grid, R.THR, False), R.draws(6, 0, G, R.SCALE, grid, R.THR, False),
                      R.draws(5, 5, G, R.SCALE, grid, R.THR, False)):
            assert float((a.cells[:M] == other.cells[:M]).mean()) < 0.02
            assert float((a.u == other.u).all(1).mean()) < 0.02


def separation(seed, c, G, grid_c):
    """(smallest max-norm distance between two draws of one cell and half, the same by x alone), in position bounds."""
    d = R.draws(seed, c, G, R.SCALE, grid_c, R.THR, False)
    bound = R.position_bound(c, G, R.SCALE)
    worst, worst_x = np.inf, np.inf
    for half in (slice(0, d.M), slice(d.M, 2 * d.M)):
        worst = min(worst, R.min_separation_within_cells(d.cells[half], d.pos[half]) / bound)
        order = np.lexsort((d.pos[half, 0], d.cells[half]))
        same = np.diff(d.cells[half][order]) == 0
        if same.any():
            worst_x = min(worst_x, float(np.diff(d.pos[half, 0][order])[same].min()) / bound)
    return worst, worst_x


@pytest.mark.parametrize("G,name,cascades", R.gpu_cases())
def test_gpu_cases_match_uniquely(G, name, cascades):
    """Any two draws of one cell lie farther apart than 64 position bounds in the max-norm, in every cascade of every GPU case,
    steady state (warm-up draws every cell once).  By x alone they do not (printed)."""
    grid0 = R.case_grid(G, name, cascades)
    seps = [separation(R.case_seed(G, name), c, G, grid0[c]) for c in range(cascades)]
    if (G, cascades) in R.REPEAT_CASES and name == "random_half":
        seps.append(separation(R.repeat_seed(G), cascades - 1, G, grid0[cascades - 1]))
    worst, worst_x = min(a for a, _ in seps), min(b for _, b in seps)
    print("G %d %s: nearest two draws of one cell: %.1f bounds apart (in x alone: %.2f)" % (G, name, worst, worst_x))
    assert worst > 64


def test_matching_finds_the_permutation():
    """match_positions on a shuffled copy moved by up to 0.9 bounds: the permutation back, and the distances."""
    G, c = 16, 3
    grid = R.pattern_grid("first_cell", 1, G, R.THR, 0, R.GRID_LO, R.GRID_HI)[0]
    d = R.draws(77, c, G, R.SCALE, grid, R.THR, False)
    bound, s = R.position_bound(c, G, R.SCALE), R.cascade_extent(c, G, R.SCALE)[0]
    rng = np.random.default_rng(0)
    perm = rng.permutation(len(d.cells))
    moved = d.pos[perm] + (rng.random((len(perm), 3)) * 2 - 1) * 0.9 * bound
    best, dist = R.match_positions(d.cells[perm], moved, d.cells, d.pos, bound, s)
    assert np.array_equal(best, perm) and dist.max() <= 0.9 * bound
    assert int(np.bincount(d.cells).max()) == d.M                      # one cell holds the whole occupied half


@pytest.mark.parametrize("G", R.FULL_PATTERN_SIZES)
def test_patterns_have_the_property_they_are_named_for(G):
    cells, words = G ** 3, G ** 3 // 64
    thr = np.float32(R.THR)
    n_neg = n_at = 0
    for name in R.PATTERNS:
        grid0 = R.case_grid(G, name, R.CASCADES)
        assert grid0.shape == (R.CASCADES, cells) and grid0.dtype == np.float32
        for c in range(R.CASCADES):
            g = grid0[c]
            occ = g > thr
            w = occ.reshape(words, 64)
            alive = g >= 0
            n_neg += int((~alive).sum()); n_at += int((g == thr).sum())
            assert ((g == -1) | ((g >= R.GRID_LO) & (g <= R.GRID_HI))).all()
            if name == "random_half":
                assert 0.3 < occ.mean() < 0.7 and (G < 16 or 0.45 < occ.mean() < 0.55)
            elif name == "all":
                assert np.array_equal(occ, alive) and occ.mean() > 0.9
            elif name == "none":
                assert not occ.any()
            elif name == "first_cell":
                assert np.array_equal(np.flatnonzero(occ), [0])
            elif name == "last_cell":
                assert np.array_equal(np.flatnonzero(occ), [cells - 1])
            elif name == "bit63_of_a_middle_word":
                assert np.array_equal(np.flatnonzero(occ), [(words // 2) * 64 + 63])
            elif name == "bit63_of_every_word":
                assert not w[:, :63].any() and (words == 1 or 0 < w[:, 63].sum()) and w[:, 63].mean() > 0.9 - (words < 64)
            elif name == "alternate_words":
                assert not w[1::2].any() and np.array_equal(w[0::2], alive.reshape(words, 64)[0::2])
            elif name == "last_word":
                assert np.array_equal(np.flatnonzero(occ), np.arange(cells - 64, cells))
        if name in ("none", "first_cell"):
            assert (grid0 == thr).any()                                  # cells exactly AT the threshold are there, and empty
    total = len(R.PATTERNS) * R.CASCADES * cells
    assert n_neg > 0 and (G < 16 or 0.01 < n_neg / total < 0.03)
    assert n_at > 0.1 * total / 2


def test_merge_and_bits_are_the_reference_projects():
    """networks.py:258-268 in torch float32: the merge bit for bit with a scalar and a per-cell decay; the threshold is Python's
    min(mean, thr), NaN mean included; the band of bits_outside_band holds exactly the cells a mean within epsilon can flip."""
    rng = np.random.default_rng(3)
    n = 4096
    g = (rng.random(n) * 3).astype(np.float32); g[rng.random(n) < 0.1] = -1.0
    tmp = (rng.random(n) * 3).astype(np.float32); tmp[rng.random(n) < 0.5] = 0.0
    for decay in (0.95, (0.1 + 0.85 * rng.random(n)).astype(np.float32)):
        tg, dk = torch.from_numpy(g), (decay if np.isscalar(decay) else torch.from_numpy(decay))
        want = torch.where(tg < 0, tg, torch.maximum(tg * dk, torch.from_numpy(tmp))).numpy()
        got = R.merge(g, tmp, decay)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got[g < 0], g[g < 0]) and 0.05 < float((got == tmp)[g >= 0].mean()) < 0.95
    mean, used, bits = R.threshold_and_bits(got, 1.0)
    assert mean == float(got[got > 0].astype(np.float64).mean()) and used == 1.0 and mean > 1.0
    assert np.array_equal(np.unpackbits(bits, bitorder="little").astype(bool), got > np.float32(1.0))
    mean, used, bits = R.threshold_and_bits(got, 1e9)
    assert used == mean and np.array_equal(np.unpackbits(bits, bitorder="little").astype(bool), got > np.float32(mean))
    mean, used, bits = R.threshold_and_bits(np.full(64, -1.0, np.float32), 1.0)
    assert mean != mean and used != used and not bits.any()
    # the band: cells planted symmetrically about 1 in steps of eps / 4; packing with the two ends of the mean's interval differs in
    # exactly the band, packing with the float64 mean differs from either end only inside it
    assert R.mean_roundings(64) == 4 and R.mean_roundings(n) == 4 and R.mean_roundings(6 * 64 ** 3) == 24 and R.mean_roundings(2 * 128 ** 3) == 64
    eps = R.mean_epsilon(n)
    assert eps == 24 * 2.0 ** -24
    k = np.arange(-40, 41)
    near = np.concatenate([1 + k * eps / 4, -np.ones(3), np.full((n - 84) // 2, 0.5), np.full((n - 84) // 2, 1.5)]).astype(np.float32)
    mean, bits, band = R.bits_outside_band(near, 1e9)
    assert abs(mean - 1) < 2.0 ** -24 and 4 <= int(band.sum()) <= 12
    lo, hi = R.packbits(near, mean * (1 - eps)), R.packbits(near, mean * (1 + eps))
    assert np.array_equal(np.unpackbits(lo ^ hi, bitorder="little").astype(bool), band)
    for end in (lo, hi):
        assert not (np.unpackbits(end ^ bits, bitorder="little").astype(bool) & ~band).any()
    _, _, band_thr = R.bits_outside_band(near, 0.5)                     # the fixed threshold wins: nothing to flip
    assert not band_thr.any()
