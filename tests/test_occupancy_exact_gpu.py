"""ngp_occupancy_update against its exact restatement (tests/occupancy_reference.py): which cells every cascade draws, where it
evaluates them, what it scatters, the merge and the packed bits.

The random stream is a counter-based integer hash, so the drawn cells are compared EXACTLY (as multisets per half: the evaluation order
is free within a block of cells), the positions within the float32 bound derived in the reference's docstring, each evaluated slot
matched one to one to a reference draw of its cell.  sigma is recomputed for the evaluated positions with the plain ngp_hashgrid_fwd +
ngp_density_fwd (pinned to the oracle in tests/test_field_gpu.py) and the scattered grid compared bit for bit: the scatter variant
is the same kernel instantiation.  The merge is bit exact.  The bits are exact wherever the device's float32 mean cannot decide
them (R.bits_outside_band; R.mean_epsilon has the derivation from density_grid_update_kernel's summation order).

Only the last cascade's cells and positions survive a call, so a case calls with cascades = 1 .. 6 on the grid's prefix, each time
from the same grid: cascade k - 1 is checked in full on call k, the scattered grids of the cascades before it against the draws and
sigmas recorded when they were last.  One workspace serves every case, never cleared.  That two draws of one cell cannot be confused
(64 bounds apart) and that every pattern is what its name says is asserted in tests/test_occupancy_reference_cpu.py on the same cases."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import occupancy_reference as R

pytestmark = pytest.mark.gpu

DECAY = 0.95
_models = {}
_ws = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from ngp_pl_amd import _lib
    return _lib


def field_params(enc):
    """Trained-like magnitudes (table O(1), not the 1e-4 init; weights 1.5 x their init), as the field fixture of
    tests/test_field_gpu.py: densities around 1.2, between 0.3 and 5."""
    g = torch.Generator().manual_seed(8)
    table = (torch.rand(enc.n_grid, generator=g) * 2 - 1) * 0.8
    return torch.cat([enc.params.detach()[:enc.n_mlp] * 1.5, table])


def model_for(G):
    """NGP(scale=16.0): six cascades; its grid resized to G^3 the way the mark-invisible test does."""
    if G not in _models:
        from ngp_pl_amd.networks import NGP
        m = NGP(scale=R.SCALE)
        assert m.cascades == R.CASCADES
        m.grid_size = G
        m.register_training_buffers()
        enc = m.xyz_encoder
        if "params" not in _models:
            _models["params"] = field_params(enc)
        with torch.no_grad():
            enc.params.copy_(_models["params"])
        _models[G] = m.cuda()
    return _models[G]


def workspace(lib):
    """One workspace for every case of this module, sized for the largest, allocated once and never cleared."""
    if "ws" not in _ws:
        need = max(lib.lib().ngp_occupancy_update_workspace_bytes(k, G) for G, _, k in R.gpu_cases())
        assert need > 0
        _ws["ws"] = torch.empty(need, dtype=torch.uint8, device="cuda")
    return _ws["ws"]


class Result:
    pass


def run_update(lib, G, grid0, thr, seed, warmup=False, decay_grid=None, evaluate=True):
    """One ngp_occupancy_update on a fresh copy of grid0 (k, G^3); what it left behind, on the host."""
    m = model_for(G)
    k, cells = grid0.shape
    assert cells == G ** 3 and 1 <= k <= m.cascades
    ws = workspace(lib)
    nbytes = lib.lib().ngp_occupancy_update_workspace_bytes(k, G)
    assert 0 < nbytes <= ws.numel()
    grid = m.density_grid[:k]
    assert grid.is_contiguous() and grid.shape == (k, cells)
    grid.copy_(torch.tensor(grid0))
    bits = torch.full((k * cells // 8,), 0xA5, dtype=torch.uint8, device="cuda")
    dg = None if decay_grid is None else torch.tensor(decay_grid).cuda()
    enc = m.xyz_encoder
    eh = enc._half.get(enc.params)
    lib.call("ngp_occupancy_update", lib.ptr(grid), lib.ptr(bits), k, G, float(R.SCALE), float(thr), DECAY, lib.ptr(dg), 1 if warmup else 0, seed,
             lib.ptr(m.xyz_min), lib.ptr(m.xyz_max), lib.ptr(eh[enc.n_mlp:]), C.byref(enc.meta), lib.ptr(eh), lib.ptr(ws), nbytes, lib.stream())
    o_tmp, o_idx, o_xyz = C.c_size_t(), C.c_size_t(), C.c_size_t()
    lib.call("ngp_occupancy_update_workspace_layout", k, G, C.byref(o_tmp), C.byref(o_idx), C.byref(o_xyz))
    n = cells if warmup else 2 * (cells // 4)
    r = Result()
    r.n, r.k = n, k
    xyz = ws[o_xyz.value:o_xyz.value + n * 12].view(torch.float32).view(n, 3).clone()
    r.idx = ws[o_idx.value:o_idx.value + n * 4].view(torch.int32).cpu().numpy().astype(np.int64)
    r.xyz = xyz.cpu().numpy()
    r.tmp = ws[o_tmp.value:o_tmp.value + k * cells * 4].view(torch.float32).view(k, cells).cpu().numpy()
    r.grid = grid.cpu().numpy()
    r.bits = bits.cpu().numpy()
    if evaluate:                                       # sigma of the evaluated positions, slot by slot, with the plain kernels
        feats = torch.empty(16, n, 2, dtype=torch.float16, device="cuda")
        sig = torch.full((n,), float("nan"), device="cuda")
        lib.call("ngp_hashgrid_fwd", lib.ptr(xyz), lib.ptr(m.xyz_min), lib.ptr(m.xyz_max), lib.ptr(eh[enc.n_mlp:]), C.byref(enc.meta), n, lib.ptr(feats), lib.stream())
        lib.call("ngp_density_fwd", lib.ptr(feats), lib.ptr(eh), n, lib.ptr(sig), None, lib.stream())
        r.sigma = sig.cpu().numpy()
        assert np.isfinite(r.sigma).all() and (r.sigma > 0).all()
    torch.cuda.synchronize()
    return r


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_draws(r, d, c, G, warmup, what):
    """Item 1.  -> (sigma per reference draw, worst position error / bound)."""
    bound, s = R.position_bound(c, G, R.SCALE), R.cascade_extent(c, G, R.SCALE)[0]
    assert r.idx.min() >= 0 and r.idx.max() < G ** 3, what
    if warmup:
        assert np.array_equal(r.idx, np.arange(G ** 3)), what
        dist = np.abs(r.xyz.astype(np.float64) - d.pos).max(1)
        assert dist.max() <= bound, "%s: position %g bounds off" % (what, dist.max() / bound)
        return r.sigma.copy(), float(dist.max() / bound)
    M, shift = d.M, R.sort_shift(G)
    sigma = np.empty(2 * M, np.float32)
    worst = 0.0
    for h, half in enumerate((slice(0, M), slice(M, 2 * M))):
        got, want = r.idx[half], d.cells[half]
        same = np.array_equal(np.sort(got), np.sort(want))
        if not same:
            a, b = np.bincount(got, minlength=G ** 3), np.bincount(want, minlength=G ** 3)
            bad = np.flatnonzero(a != b)
            raise AssertionError("%s half %d: the evaluated cells are not the drawn cells: %d cells differ in count, first %d: evaluated %d times, drawn %d times"
                                 % (what, h, len(bad), bad[0], a[bad[0]], b[bad[0]]))
        assert (np.diff(got >> shift) >= 0).all(), "%s half %d: evaluation order is not by block of 2^%d cells" % (what, h, shift)
        best, dist = R.match_positions(got, r.xyz[half], want, d.pos[half], bound, s)
        assert (best >= 0).all() and dist.max() <= bound, "%s half %d: %d evaluated positions are not a draw of their cell (worst %g bounds)" % (
            what, h, int((dist > bound).sum()), dist.max() / bound)
        assert len(np.unique(best)) == M, "%s half %d: two slots evaluate the same draw" % (what, h)
        sigma[half.start + best] = r.sigma[half]
        worst = max(worst, float(dist.max() / bound))
    return sigma, worst


class Record:
    """The draws of one cascade with the sigma of each, grouped by cell once for the scatter checks of the later calls."""

    def __init__(self, cells, sigma, G):
        order = np.argsort(cells, kind="stable")
        self.cells, self.sigma = cells[order], u32(sigma)[order]
        self.uniq, self.start = np.unique(self.cells, return_index=True)
        self.never = np.ones(G ** 3, bool)
        self.never[self.uniq] = False


def check_scatter(tmp_c, rec, what):
    """Item 2: tmp[cell] is bit-equal to the sigma of one of the cell's draws, +0 where nothing was drawn."""
    t = u32(tmp_c)
    ok = np.logical_or.reduceat(t[rec.cells] == rec.sigma, rec.start)
    if not ok.all():
        cell = rec.uniq[np.flatnonzero(~ok)[0]]
        raise AssertionError("%s: %d drawn cells hold a density that is none of their draws'; first cell %d: holds %r, draws %r"
                             % (what, int((~ok).sum()), cell, float(tmp_c[cell]), rec.sigma[rec.cells == cell][:8].view(np.float32).tolist()))
    assert not t[rec.never].any(), "%s: a cell that was not drawn is not +0" % what


def check_merge_and_bits(r, grid0, thr, decay, what):
    """Items 3 and 6 (4 where the threshold wins).  -> (share of merges sigma wins, band population)."""
    want = R.merge(grid0, r.tmp, decay)
    diff = u32(r.grid) != u32(want)
    assert not diff.any(), "%s: %d merged cells differ, first %d" % (what, int(diff.sum()), np.flatnonzero(diff.reshape(-1))[0])
    neg = grid0 < 0
    assert np.array_equal(u32(r.grid)[neg], u32(grid0)[neg])
    mean, bits, band = R.bits_outside_band(r.grid, thr)
    wrong = np.unpackbits(bits ^ r.bits, bitorder="little").astype(bool) & ~band
    assert not wrong.any(), "%s: %d bits differ outside the band of the mean %r" % (what, int(wrong.sum()), mean)
    assert band.mean() <= 1e-4, "%s: %d cells within epsilon of the mean" % (what, int(band.sum()))
    live = (r.tmp != 0) & ~neg
    return (int((r.grid == r.tmp)[live].sum()), int(live.sum())), int(band.sum())


@pytest.mark.parametrize("G,name,cascades", R.gpu_cases())
def test_steady_state_update_is_the_reference(lib, G, name, cascades):
    """Items 1-3 and 6 for every cascade count, once with the scalar decay and once with a per-cell decay grid."""
    grid0 = R.case_grid(G, name, cascades)
    seed = R.case_seed(G, name)
    rng = np.random.default_rng(G)
    decay_grid = (0.1 + 0.85 * rng.random(grid0.shape)).astype(np.float32)
    records = {}
    won = total = band_cells = 0
    worst = 0.0
    for k in range(1, cascades + 1):
        what = "G %d %s, %d cascades" % (G, name, k)
        r = run_update(lib, G, grid0[:k], R.THR, seed)
        c = k - 1
        d = R.draws(seed, c, G, R.SCALE, grid0[c], R.THR, False)
        sigma, w = check_draws(r, d, c, G, False, what)
        worst = max(worst, w)
        records[c] = Record(d.cells, sigma, G)
        for cc in range(k):
            check_scatter(r.tmp[cc], records[cc], "%s, cascade %d" % (what, cc))
        (a, b), nb = check_merge_and_bits(r, grid0[:k], R.THR, DECAY, what)
        won, total, band_cells = won + a, total + b, band_cells + nb
        # the per-cell decay: same draws (they depend on grid0 alone), its own merge
        r2 = run_update(lib, G, grid0[:k], R.THR, seed, decay_grid=decay_grid[:k], evaluate=False)
        assert np.array_equal(r2.idx[:d.M] >> R.sort_shift(G), r.idx[:d.M] >> R.sort_shift(G))
        for cc in range(k):
            check_scatter(r2.tmp[cc], records[cc], "%s, per-cell decay, cascade %d" % (what, cc))
        (a, b), nb = check_merge_and_bits(r2, grid0[:k], R.THR, decay_grid[:k], what + ", per-cell decay")
        won, total, band_cells = won + a, total + b, band_cells + nb
    print("G %d %s: worst position error %.3f bounds; sigma wins %.1f %% of %d merges; %d cells in the mean's band" % (G, name, worst, 100.0 * won / total, total, band_cells))
    assert 0.05 < won / total < 0.95, (won, total)


@pytest.mark.parametrize("G,cascades", [(4, 6), (8, 6), (16, 6), (32, 6), (64, 6), (128, 2)])
def test_warmup_update_is_the_reference(lib, G, cascades):
    """Warm-up: every cell once and in order, positions by slot, every cascade's scattered grid the sigma of its own positions."""
    grid0 = R.case_grid(G, "random_half", cascades)
    seed = R.case_seed(G, "all") + 1
    kept = {}
    worst = 0.0
    for k in range(1, cascades + 1):
        what = "warm-up G %d, %d cascades" % (G, k)
        r = run_update(lib, G, grid0[:k], R.THR, seed, warmup=True)
        c = k - 1
        d = R.draws(seed, c, G, R.SCALE, grid0[c], R.THR, True)
        sigma, w = check_draws(r, d, c, G, True, what)
        worst = max(worst, w)
        kept[c] = sigma
        for cc in range(k):                              # no cell is drawn twice: bit for bit
            assert np.array_equal(u32(r.tmp[cc]), u32(kept[cc])), "%s, cascade %d" % (what, cc)
        check_merge_and_bits(r, grid0[:k], R.THR, DECAY, what)
    print("warm-up G %d: worst position error %.3f bounds" % (G, worst))


@pytest.mark.parametrize("G,cascades", [(4, 6), (64, 6), (128, 2)])
def test_bits_where_the_threshold_wins(lib, G, cascades):
    """Item 4: thr = 2.0 far below the mean of the positive cells: the bits are packbits(grid, thr), exactly."""
    thr = 2.0
    grid0 = R.pattern_grid("random_half", cascades, G, thr, seed=G + 1, lo=0.0, hi=40.0)
    r = run_update(lib, G, grid0, thr, seed=R.case_seed(G, "all") + 2, evaluate=False)
    assert np.array_equal(u32(r.grid), u32(R.merge(grid0, r.tmp, DECAY)))
    assert R.positive_mean(r.grid) > 2 * thr
    assert np.array_equal(r.bits, R.packbits(r.grid, thr))
    assert 0.3 < np.unpackbits(r.bits).mean() < 0.7


def two_cluster_grid(G, cascades, seed):
    rng = np.random.default_rng(seed)
    n = cascades * G ** 3
    high = rng.random(n) < 0.5
    g = np.where(high, 800 + 200 * rng.random(n), 100 + 100 * rng.random(n)).astype(np.float32)
    g[rng.random(n) < 0.02] = -1.0
    g[0], g[n - 1] = 1000.0, 100.0
    return g.reshape(cascades, G ** 3)


@pytest.mark.parametrize("G,cascades", [(4, 1), (4, 6), (16, 6), (64, 6), (128, 2)])
def test_bits_where_the_mean_wins_and_is_known(lib, G, cascades):
    """Item 5: every cell -1 or in [100, 200] u [800, 1000] and every sigma below 95, so the merge is g * 0.95 exactly; with thr = 1e9
    the threshold is the mean, which falls in the gap between the clusters whatever its rounding: the bits are the high cluster."""
    grid0 = two_cluster_grid(G, cascades, seed=G + cascades)
    r = run_update(lib, G, grid0, 1e9, seed=R.case_seed(G, "all") + 3, evaluate=False)
    assert r.tmp.max() < 95 and r.tmp.max() > 0
    want = R.merge(grid0, np.zeros_like(grid0), DECAY)
    assert np.array_equal(u32(r.grid), u32(want))
    mean = R.positive_mean(want)
    assert 190 * 1.01 < mean < 760 * 0.99
    high = (grid0 >= 800).reshape(-1)
    assert 0.3 < high.mean() < 0.7 or G == 4
    assert np.array_equal(np.unpackbits(r.bits, bitorder="little").astype(bool), high)
    assert np.array_equal(r.bits, R.packbits(want, mean))


@pytest.mark.parametrize("G,cascades", [(4, 1), (4, 6), (32, 6), (64, 6), (128, 2)])
def test_bits_where_the_mean_wins(lib, G, cascades):
    """Item 6: thr = 1e9 on the random-half grid: the threshold is the device's own float32 mean.  Bits may differ from
    packbits(grid, mean64) only at cells within epsilon = (L + 20) 2^-24 of the mean, L = R.mean_roundings; at most 1e-4 of the cells
    lie there, every other bit is exact (both asserted in check_merge_and_bits)."""
    grid0 = R.case_grid(G, "random_half", cascades)
    r = run_update(lib, G, grid0, 1e9, seed=R.case_seed(G, "all") + 4, evaluate=False)
    _, nb = check_merge_and_bits(r, grid0, 1e9, DECAY, "G %d, %d cascades, thr 1e9" % (G, cascades))
    mean = R.positive_mean(r.grid)
    share = np.unpackbits(r.bits).mean()
    print("G %d x %d: L = %d, epsilon %.3g, mean %.6f, %d of %d cells in the band" % (G, cascades, R.mean_roundings(r.grid.size), R.mean_epsilon(r.grid.size), mean, nb, r.grid.size))
    assert 0.2 < share < 0.8                                          # the mean splits the cells: neither all nor none


@pytest.mark.parametrize("G,cascades", [(4, 1), (16, 6), (128, 2)])
@pytest.mark.parametrize("warmup", [False, True])
def test_all_cells_invisible(lib, G, cascades, warmup):
    """Item 7: every cell -1: the mean is 0 / 0, every bit is 0 and the grid is unchanged."""
    grid0 = np.full((cascades, G ** 3), -1.0, np.float32)
    r = run_update(lib, G, grid0, R.THR, seed=9, warmup=warmup, evaluate=False)
    assert np.array_equal(u32(r.grid), u32(grid0))
    assert not r.bits.any()
    if not warmup:
        assert (r.idx[G ** 3 // 4:] == G ** 3 - 1).all()


@pytest.mark.parametrize("G,cascades", R.REPEAT_CASES)
def test_two_identical_calls_agree(lib, G, cascades):
    """Item 8: the workspace is whatever the cases before left in it.  Cells drawn more than once may keep another draw's sigma from
    call to call: there both calls must hold one of the cell's sigmas (checked in full for the last cascade), everywhere else every
    bit of tmp, grid and bitfield agrees."""
    grid0 = R.case_grid(G, "random_half", cascades)
    seed = R.repeat_seed(G)
    a = run_update(lib, G, grid0, R.THR, seed)
    b = run_update(lib, G, grid0, R.THR, seed)
    c = cascades - 1
    d = R.draws(seed, c, G, R.SCALE, grid0[c], R.THR, False)
    for r in (a, b):
        sigma, _ = check_draws(r, d, c, G, False, "G %d" % G)
        check_scatter(r.tmp[c], Record(d.cells, sigma, G), "G %d" % G)
        check_merge_and_bits(r, grid0, R.THR, DECAY, "G %d" % G)
    assert np.array_equal(a.tmp != 0, b.tmp != 0)
    assert np.array_equal(np.sort(a.idx[:d.M]), np.sort(b.idx[:d.M])) and np.array_equal(np.sort(a.idx[d.M:]), np.sort(b.idx[d.M:]))
    differ = u32(a.tmp) != u32(b.tmp)
    once = np.ones_like(differ)
    for cc in range(cascades):
        dd = d if cc == c else R.draws(seed, cc, G, R.SCALE, grid0[cc], R.THR, False)
        once[cc] = np.bincount(dd.cells, minlength=G ** 3) <= 1
    assert not (differ & once).any()
    assert np.array_equal(u32(a.grid)[~differ], u32(b.grid)[~differ])
    if not differ.any():
        assert np.array_equal(a.bits, b.bits)
    print("G %d: %d cells drawn twice hold another draw's sigma in the second call" % (G, int(differ.sum())))
