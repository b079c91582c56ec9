"""TEST INFRASTRUCTURE -- inputs of the exact table-backward tests (tests/test_table_backward_reference_cpu.py runs on the CPU,
tests/test_table_backward_exact_gpu.py on the GPU) and the conditions those inputs must meet, evaluated on the reference's terms.

The two constants below are the only knowledge of the binned kernel in here: they say WHERE its paths change (a slice of the table
per task, a block of samples per binning workgroup), so that the inputs can be shown to reach every path."""
import math
from types import SimpleNamespace

import numpy as np
import torch

SLICE = 6912          # table entries per slice owner task
BLOCK = 1024          # samples per binning workgroup

# name -> (n_levels, log2_hashmap_size, base_resolution, per_level_scale, half extent of the box)
GRIDS = {
    "product": (16, 19, 16, math.exp(math.log(2048 * 0.5 / 16) / 15), 0.5),
    "scale16": (16, 19, 16, math.exp(math.log(2048 * 16 / 16) / 15), 16.0),
    # resolutions 16, 21, 26 dense (4096, 9264, 17576 entries: one, two and three slices), 33 .. 81 hashed into 2^15 = 4 slices + 5120
    "small": (8, 15, 16, 1.26, 2.0),
}


def grid_arrays(meta, name):
    """meta: anything with .resolution / .offset / .scale per level (the native record or the oracle's GridMeta)."""
    n_levels, half = GRIDS[name][0], GRIDS[name][4]
    return SimpleNamespace(name=name, n_levels=n_levels, half=half,
                           resolution=[int(meta.resolution[l]) for l in range(n_levels)],
                           offset=[int(meta.offset[l]) for l in range(n_levels + 1)],
                           scale=[float(meta.scale[l]) for l in range(n_levels)],
                           xyz_min=np.full(3, -half, np.float32), xyz_max=np.full(3, half, np.float32))


def native_grid(name):
    """The level table the kernels are given (ngp_grid_meta_init: host code, needs no GPU).  Returns (arrays, native record)."""
    import ctypes as C
    from ngp_pl_amd import _lib
    n_levels, log2_size, base, b, _ = GRIDS[name]
    meta = _lib.GridMeta()
    _lib.call("ngp_grid_meta_init", C.byref(meta), n_levels, 2, log2_size, base, float(b))
    return grid_arrays(meta, name), meta


def level_sizes(grid):
    return [grid.offset[l + 1] - grid.offset[l] for l in range(grid.n_levels)]


def dense_levels(grid):
    return [l for l, s in enumerate(level_sizes(grid)) if grid.resolution[l] ** 3 <= s]


def make_points(n, half, seed):
    """Uniform points; ray-like runs of 100 collinear points 1.7e-3 of the extent apart in front (200 runs once n allows it, else half
    of the points); the 8 closed box corners (x01 = 0 and 1 on every axis) at the end."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, 3, generator=g) - 0.5) * (2 * half)
    runs = 200 if n >= 20008 else n // 200
    if runs:
        o = (torch.rand(runs, 1, 3, generator=g) - 0.5) * (2 * half)
        dd = torch.randn(runs, 1, 3, generator=g)
        dd /= dd.norm(dim=-1, keepdim=True)
        x[:runs * 100] = (o + dd * (torch.arange(100).view(1, 100, 1) * (1.7e-3 * 2 * half))).clamp(-half, half).reshape(-1, 3)
    if n >= runs * 100 + 8:
        for c in range(8):
            x[n - 8 + c] = torch.tensor([half if (c >> k) & 1 else -half for k in range(3)])
    elif n >= 1:
        x[n - 1] = torch.tensor([half, -half, half])
    return x.contiguous()


def make_seeds(n, n_levels, seed):
    """(n_levels, n, 2) f16 upstream gradients: magnitudes log-uniform from 2^-24 (the smallest f16 subnormal) to 30 000, both signs;
    rows with (0, 0), (-0.0, 0.0), (0, g1) and (g0, 0); the two extremes planted in rows 1 and 2."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = math.log(2.0 ** -24), math.log(30000.0)
    mag = torch.exp(torch.rand(n_levels, n, 2, generator=g) * (hi - lo) + lo)
    d = (mag * torch.where(torch.rand(n_levels, n, 2, generator=g) < 0.5, -1.0, 1.0)).half()
    r = torch.arange(n) % 16
    d[:, r == 3] = 0
    d[:, r == 5] = torch.tensor([-0.0, 0.0], dtype=torch.float16)
    d[:, r == 7, 0] = 0
    d[:, r == 9, 1] = 0
    if n >= 3:
        d[:, 1, 0] = 2.0 ** -24
        d[:, 2, 1] = 30000.0
    return d.contiguous()


def seeds_cover_the_range(d):
    """(0,0) rows, (-0.0, 0.0) rows, one-sided rows, the subnormal 2^-24 and 30 000 are all in the batch."""
    a = d.float().abs()
    neg_zero = (d[..., 0].view(torch.int16) == -32768) & (d[..., 1].view(torch.int16) == 0)
    plain_zero = (d[..., 0].view(torch.int16) == 0) & (d[..., 1].view(torch.int16) == 0)
    return bool(neg_zero.any() and plain_zero.any() and ((a[..., 0] == 0) & (a[..., 1] > 0)).any() and ((a[..., 0] > 0) & (a[..., 1] == 0)).any()
                and float(a[a > 0].min()) == 2.0 ** -24 and float(a.max()) == 30000.0)


def make_crowd(grid, n, seed):
    """n points inside ONE cell of the finest level that also lies inside one cell of every dense level."""
    s_fine = np.float64(grid.scale[grid.n_levels - 1])
    coarse = [np.float64(grid.scale[l]) for l in dense_levels(grid)]
    rng = np.random.RandomState(seed)
    ks = []
    for first in (0.31, 0.47, 0.62):                                 # per axis: the first finest-level cell from there on that fits
        for k in range(int(first * s_fine), int(s_fine)):
            lo, hi = (k - 0.45) / s_fine, (k + 0.45) / s_fine        # pos = x01 * scale + 0.5 stays in [k + 0.05, k + 0.95]
            if all(np.floor(lo * s + 0.5) == np.floor(hi * s + 0.5) for s in coarse):
                ks.append(k)
                break
    assert len(ks) == 3, "no finest-level cell inside one cell of every dense level"
    k = np.array(ks, np.float64)
    x01 = (k - 0.45) / s_fine + rng.rand(n, 3) * (0.9 / s_fine)
    return torch.from_numpy((x01 * 2 * grid.half - grid.half).astype(np.float32)).contiguous()


def make_active(n_x, m, seed):
    """m indices out of range(n_x), strictly increasing (what ngp_active_samples produces: ray order)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(n_x, generator=g)[:m].sort().values.int().contiguous()


# ---- conditions on the inputs, evaluated on the reference's terms ------------------------------------------------------------------
def straddling_pairs(ref):
    """Hashed corner pairs (x, .), (x + 1, .) whose two indices fall into different slices."""
    n = 0
    for lv in ref.levels:
        if lv.hashed:
            for k in range(4):
                n += int((lv.idx[2 * k] // SLICE != lv.idx[2 * k + 1] // SLICE).sum())
    return n


def max_contributions_of_one_block(ref):
    """Largest number of contributions that one hashed entry receives from the samples of one block."""
    best = 0
    for lv in ref.levels:
        if lv.hashed and lv.j.size:
            key = np.concatenate([(lv.j // BLOCK) * lv.size + lv.idx[c] for c in range(8)])
            best = max(best, int(np.unique(key, return_counts=True)[1].max()))
    return best


def dense_levels_hold_one_cell(ref):
    dense = [lv for lv in ref.levels if not lv.hashed]
    return bool(dense) and all(lv.j.size > 0 and bool((lv.cell == lv.cell[0]).all()) for lv in dense)


def dense_split_branches(grid):
    """Which of the three dense table sizes (one slice, two slices, more) the grid has."""
    sizes = [level_sizes(grid)[l] for l in dense_levels(grid)]
    return (any(s <= SLICE for s in sizes), any(SLICE < s <= 2 * SLICE for s in sizes), any(s > 2 * SLICE for s in sizes))


def has_partial_last_slice(grid):
    d = set(dense_levels(grid))
    return any(s % SLICE != 0 for l, s in enumerate(level_sizes(grid)) if l not in d)


# ---- the cases: inputs and their reference, computed once and shared ----------------------------------------------------------------
_CASES = {}


def reference_of(grid, x, d, active_idx=None, n_active=None):
    from tests import table_backward_reference as R
    return R.table_backward_reference(x.numpy(), grid.xyz_min, grid.xyz_max, d.numpy(), grid.resolution, grid.offset, grid.scale,
                                      None if active_idx is None else active_idx.numpy(), n_active)


def plain_case(name, n):
    """n points / seeds on grid `name` and the reference of the whole batch."""
    key = ("plain", name, n)
    if key not in _CASES:
        grid, meta = native_grid(name)
        x = make_points(n, grid.half, seed=100 + n)
        d = make_seeds(n, grid.n_levels, seed=200 + n)
        _CASES[key] = SimpleNamespace(grid=grid, meta=meta, x=x, d=d, ref=reference_of(grid, x, d))
    return _CASES[key]


def crowd_case(name, n, big):
    """n points in one finest-level cell; big: every gradient +60 000."""
    key = ("crowd", name, n, big)
    if key not in _CASES:
        grid, meta = native_grid(name)
        x = make_crowd(grid, n, seed=7)
        d = torch.full((grid.n_levels, n, 2), 60000.0, dtype=torch.float16) if big else make_seeds(n, grid.n_levels, seed=8)
        _CASES[key] = SimpleNamespace(grid=grid, meta=meta, x=x, d=d, ref=reference_of(grid, x, d))
    return _CASES[key]
