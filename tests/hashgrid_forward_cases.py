"""TEST INFRASTRUCTURE -- inputs of the exact hash-forward tests (tests/test_hashgrid_forward_reference_cpu.py on the CPU,
tests/test_hashgrid_forward_exact_gpu.py on the GPU) and the conditions those inputs must meet, evaluated on the reference's terms
(tests/hashgrid_forward_reference.py: cells per level), never on the kernel's.

The constants WAVE and CHUNK are the only knowledge of the kernels in here: they say where a kernel's paths change (a cell run is
looked for inside a wave of 64 consecutive samples, a workgroup takes 256), so that the inputs can be shown to reach them."""
import functools
import math
from types import SimpleNamespace

import numpy as np

from tests import hashgrid_forward_reference as F
from tests import table_backward_cases as K

WAVE, CHUNK = 64, 256
STEP = 1.7e-3                                 # a march step, as a share of the box extent

# name -> (n_levels, log2_hashmap_size, base_resolution, per_level_scale, half extent of the symmetric box)
GRIDS = {name: K.GRIDS[name] for name in ("product", "scale16", "small")}
# 12 levels, resolutions 16 .. 1384: four dense levels, eight hashed ones of 2 MiB -- the cost-balanced workgroup map with fewer than 16
# levels (host-sized launch), level = xcd + 8 * slot with slot 1 half empty (device-sized and list launches)
GRIDS["levels12"] = (12, 19, 16, 1.5, 1.0)
# 4 levels, resolutions 16, 32 (32^3 = 2^15: a dense level that fills the cap exactly), 64, 128 hashed: XCDs 4 .. 7 have no level
GRIDS["levels4"] = (4, 15, 16, 2.0, 0.5)
EXACT = "product_exact"                        # the product grid with level_table="exact" (resolutions 64 / 256 / 1024 at levels 5 / 10 / 15)
GRID_NAMES = tuple(GRIDS) + (EXACT,)

BOX_NAMES = ("sym", "skew")
SKEW = (np.array([-1.0, 0.0, -16.0], np.float32), np.array([3.0, 0.5, 16.0], np.float32))       # extents 4, 0.5, 32

TABLE_NAMES = ("uniform", "log")
SET_NAMES = ("march", "axes", "repeat", "abab", "faces", "corners", "outside")
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 4097)
MARCH_RAYS, RAY_LEN = 41, 100                  # 4100 samples: every count is a prefix


@functools.lru_cache(maxsize=None)
def grid_of(name):
    """(arrays, native record) of a grid: the level table the kernels are given (host code, needs no GPU)."""
    import ctypes as C
    from ngp_pl_amd import _lib
    if name == EXACT:
        from ngp_pl_amd import tcnn
        n_levels, log2_size, base, b, half = GRIDS["product"]
        meta = tcnn.make_grid_meta({"otype": "Grid", "type": "Hash", "n_levels": n_levels, "n_features_per_level": 2, "log2_hashmap_size": log2_size,
                                    "base_resolution": base, "per_level_scale": b, "interpolation": "Linear"}, level_table="exact")
    else:
        n_levels, log2_size, base, b, half = GRIDS[name]
        meta = _lib.GridMeta()
        _lib.call("ngp_grid_meta_init", C.byref(meta), n_levels, 2, log2_size, base, float(b))
    arrays = SimpleNamespace(name=name, n_levels=n_levels, half=half,
                             resolution=[int(meta.resolution[l]) for l in range(n_levels)],
                             offset=[int(meta.offset[l]) for l in range(n_levels + 1)],
                             scale=[float(meta.scale[l]) for l in range(n_levels)])
    return arrays, meta


def box_of(grid, box):
    if box == "sym":
        return np.full(3, -grid.half, np.float32), np.full(3, grid.half, np.float32)
    return SKEW


def level_sizes(grid):
    return [grid.offset[l + 1] - grid.offset[l] for l in range(grid.n_levels)]


def dense_levels(grid):
    return [l for l, s in enumerate(level_sizes(grid)) if grid.resolution[l] ** 3 <= s]


def hashed_levels(grid):
    d = set(dense_levels(grid))
    return [l for l in range(grid.n_levels) if l not in d]


def face_levels(grid):
    """Level 0, the last dense, the first hashed and the last level."""
    return sorted({0, dense_levels(grid)[-1], hashed_levels(grid)[0], grid.n_levels - 1})


@functools.lru_cache(maxsize=None)
def table_of(name, kind):
    """(total, 2) f16.  uniform: +-0.8.  log: magnitudes log-uniform from 2^-24 (the smallest f16 subnormal) to 30 000, both signs:
    subnormal outputs and cancellation, and no overflow because the weights of a sample sum to 1."""
    total = grid_of(name)[0].offset[-1]
    rng = np.random.RandomState(GRID_NAMES.index(name) * 2 + TABLE_NAMES.index(kind) + 900)
    if kind == "uniform":
        return ((rng.rand(total, 2) * 2 - 1) * 0.8).astype(np.float16)
    lo, hi = math.log(2.0 ** -24), math.log(30000.0)
    mag = np.exp(rng.rand(total, 2) * (hi - lo) + lo)
    t = (mag * np.where(rng.rand(total, 2) < 0.5, -1.0, 1.0)).astype(np.float16)
    t[0], t[1] = (2.0 ** -24, -30000.0), (30000.0, -2.0 ** -24)                                 # the two extremes, in level 0
    return t


# ---- point sets, built in unit coordinates and carried into the box -------------------------------------------------------------------
def to_box(u, mn, mx):
    return (mn.astype(np.float64) + np.asarray(u, np.float64) * (mx.astype(np.float64) - mn.astype(np.float64))).astype(np.float32)


def march_rays(n_rays, seed):
    """Rays of RAY_LEN samples, STEP of the extent apart, clamped to the closed box."""
    rng = np.random.RandomState(seed)
    o = rng.rand(n_rays, 1, 3) * 0.7 + 0.15
    d = rng.randn(n_rays, 1, 3)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.clip(o + d * (np.arange(RAY_LEN).reshape(1, RAY_LEN, 1) * STEP), 0.0, 1.0).reshape(-1, 3)


def axis_rays():
    """Three rays of 200 samples, each along one axis alone: the other two coordinates do not move."""
    u = np.empty((3, 200, 3))
    for a in range(3):
        u[a] = np.array([0.23, 0.31, 0.42])
        u[a, :, a] = 0.3 + np.arange(200) * STEP
    return u.reshape(-1, 3)


def face_points(grid, mn, mx):
    """Per level of face_levels, axis and face j (pos = j, x01 = (j - 0.5) / scale; j = 1, 2, 3, res / 2 and the last two faces inside
    the box, res - 1 where the box reaches it): the five consecutive f32 values of x around the face -- the f32 positions the kernel
    can be GIVEN there (consecutive x01 need not all be reachable from an x) -- as five neighbouring samples; the other two coordinates
    sit inside a cell.  Eight groups of five per level and axis: six faces, and two more groups next to face 1."""
    rng = np.random.RandomState(77)
    pts = []
    for l in face_levels(grid):
        s, res = np.float64(np.float32(grid.scale[l])), grid.resolution[l]
        j_max = min(res - 1, int(math.floor(s + 0.5)))
        for a in range(3):
            for j in sorted({1, 2, 3, res // 2, j_max - 1, j_max}):
                x0 = to_box((j - 0.5) / s, mn[a:a + 1], mx[a:a + 1])[0]
                xs = [x0]
                for _ in range(2):
                    xs = [np.nextafter(xs[0], np.float32(-np.inf))] + xs + [np.nextafter(xs[-1], np.float32(np.inf))]
                p = to_box(np.repeat(rng.rand(1, 3) * 0.8 + 0.1, 5, axis=0), mn, mx)
                p[:, a] = np.clip(np.array(xs, np.float32), mn[a], mx[a])
                pts.append(p)
            # face 1 once more, the next five values to either side: x01 * scale = 0.5 lies one binade below pos = 1, the one face
            # where rounding the product first can choose the other cell
            for side in (-1.0, 1.0):
                xs = [to_box(0.5 / s, mn[a:a + 1], mx[a:a + 1])[0]]
                for _ in range(7):
                    xs.append(np.nextafter(xs[-1], np.float32(side * np.inf)))
                p = to_box(np.repeat(rng.rand(1, 3) * 0.8 + 0.1, 5, axis=0), mn, mx)
                p[:, a] = np.array(xs[3:], np.float32)
                pts.append(p)
    return np.concatenate(pts)


def outside_points(seed=5):
    """512 points up to 4 x the half extent away from the centre, both signs, in groups of 3 between groups of 5 points inside."""
    rng = np.random.RandomState(seed)
    u = rng.rand(512, 3)
    out = (np.arange(512) % 8) >= 5
    u[out] = u[out] * 4.0 - 1.5
    u[5] = (-1.5, 2.5, -1.5)
    u[6] = (2.5, -1.5, 2.5)
    return u


@functools.lru_cache(maxsize=None)
def points_of(name, box, which):
    """x (n, 3) f32 of point set `which` for grid `name` in box `box`."""
    grid = grid_of(name)[0]
    mn, mx = box_of(grid, box)
    if which == "march":
        return to_box(march_rays(MARCH_RAYS, seed=3), mn, mx)
    if which == "march_long":
        return to_box(march_rays(400, seed=4), mn, mx)
    if which == "axes":
        return to_box(axis_rays(), mn, mx)
    if which == "repeat":
        return to_box(np.repeat(np.array([[0.37, 0.52, 0.61]]), 300, axis=0), mn, mx)
    if which == "abab":
        return to_box(np.array([[0.3, 0.3, 0.3], [0.7, 0.6, 0.4]])[np.arange(130) % 2], mn, mx)
    if which == "faces":
        return face_points(grid, mn, mx)
    if which == "corners":
        return to_box(np.array([[(c >> k) & 1 for k in range(3)] for c in range(8)], np.float64), mn, mx)
    if which == "outside":
        return to_box(outside_points(), mn, mx)
    raise KeyError(which)


@functools.lru_cache(maxsize=24)
def reference_of(name, box, which, table):
    """The forward reference of a point set, computed once and shared."""
    grid = grid_of(name)[0]
    mn, mx = box_of(grid, box)
    return F.forward_reference(points_of(name, box, which), mn, mx, table_of(name, table), grid.resolution, grid.offset, grid.scale, grid.n_levels)


def reference_rows(name, box, which, table, rows):
    """The same for some rows of a point set (not cached)."""
    grid = grid_of(name)[0]
    mn, mx = box_of(grid, box)
    return F.forward_reference(points_of(name, box, which)[rows], mn, mx, table_of(name, table), grid.resolution, grid.offset, grid.scale, grid.n_levels)


# ---- conditions on the inputs, evaluated on the reference's cells ------------------------------------------------------------------------
def same_cell_as_next(cell):
    """(n - 1,) bool: sample i and i + 1 share their cell."""
    return (cell[1:] == cell[:-1]).all(axis=1)


def run_spans_a_wave_boundary(cell):
    same = same_cell_as_next(cell)
    return bool(same[WAVE - 1::WAVE].any())


def share_of_neighbours_that_differ(cell):
    return float(1.0 - same_cell_as_next(cell).mean())


def neighbours_differ_in_one_coordinate_only(cell, axis):
    d = cell[1:] != cell[:-1]
    others = [k for k in range(3) if k != axis]
    return bool((d[:, axis] & ~d[:, others[0]] & ~d[:, others[1]]).any())


def signed(cell):
    return cell.astype(np.int64) - ((cell.astype(np.int64) >> 31) << 32)


def count_with_last_sample_alone(ref):
    """The smallest n > CHUNK, not a multiple of the wave, whose last sample shares its cell with its predecessor on NO level."""
    alone = np.ones(ref.n - 1, bool)
    for lv in ref.levels:
        alone &= ~same_cell_as_next(lv.cell)
    for i in range(CHUNK, ref.n - 1):
        if alone[i] and (i + 2) % WAVE > 1:
            return i + 2                                               # samples 0 .. i + 1
    raise AssertionError("no such count")


def count_that_cuts_a_run_mid_wave(ref):
    """The smallest n > 2 * CHUNK, not a multiple of the wave, at which sample n - 1 and sample n share their cell on level 0."""
    same = same_cell_as_next(ref.levels[0].cell)
    for n in range(2 * CHUNK + 1, ref.n):
        if same[n - 1] and same[n - 2] and n % WAVE:
            return n
    raise AssertionError("no such count")


def counts_of(ref):
    return COUNTS + (count_with_last_sample_alone(ref), count_that_cuts_a_run_mid_wave(ref))


def check_conditions(name, box, which):
    """Raises AssertionError unless point set `which` reaches what it is built for on grid `name` in box `box`."""
    grid = grid_of(name)[0]
    ref = reference_of(name, box, which, "uniform")
    lv = ref.levels
    dense, hashed = dense_levels(grid), hashed_levels(grid)
    assert dense and hashed and dense[-1] + 1 == hashed[0]
    inside = all(bool((signed(v.cell) >= 0).all() and (signed(v.cell) <= v.res - 1).all()) for v in lv)
    if which == "march":
        assert ref.n == MARCH_RAYS * RAY_LEN >= max(COUNTS) and inside
        assert run_spans_a_wave_boundary(lv[0].cell)
        share = share_of_neighbours_that_differ(lv[-1].cell)
        # a step is STEP * scale cells long: on the recipe grids (finest scale >= 1023) most neighbours sit in different cells
        assert share > (0.5 if grid.scale[-1] * STEP > 1.0 else 0.05), share
        n_alone, n_cut = counts_of(ref)[-2:]
        assert CHUNK < n_alone < ref.n and all(not same_cell_as_next(v.cell)[n_alone - 2] for v in lv)
        assert n_cut % WAVE and same_cell_as_next(lv[0].cell)[n_cut - 1]
    elif which == "axes":
        assert inside
        for a in range(3):
            for v in (lv[0], lv[-1]):
                assert neighbours_differ_in_one_coordinate_only(v.cell[200 * a:200 * (a + 1)], a), (a, v.res)
    elif which == "repeat":
        assert ref.n > CHUNK and inside and all(bool((v.cell == v.cell[0]).all()) for v in lv)
    elif which == "abab":
        for v in lv:
            assert ref.n > WAVE and not same_cell_as_next(v.cell).any() and bool((v.cell[2:] == v.cell[:-2]).all())
    elif which == "faces":
        assert inside
        n_faces = ref.n // 5
        per_level = n_faces // len(face_levels(grid))
        both, zero = 0, 0
        for k, l in enumerate(face_levels(grid)):
            for g in range(k * per_level, (k + 1) * per_level):
                a = (g - k * per_level) // (per_level // 3)
                c, f = lv[l].cell[5 * g:5 * g + 5, a], lv[l].f[5 * g:5 * g + 5, a]
                both += int(c.min() + 1 == c.max())
                zero += int((f == 0).any())
            assert (lv[l].cell == 1).any() and (lv[l].cell == min(lv[l].res - 1, int(math.floor(lv[l].scale + 0.5)))).any()
        assert both >= n_faces // 2 and zero >= 1, (both, zero, n_faces)   # both sides of a face among five neighbours; f = 0 exactly
    elif which == "corners":
        assert ref.n == 8 and inside
        for v in lv:
            assert bool((v.cell.min(axis=0) == 0).all()) and bool((v.f[0] == 0.5).all())
            top = v.pos.max(axis=0)
            assert bool((top == np.float32(v.scale) + np.float32(0.5)).all()) or v.scale >= 2.0 ** 23
    elif which == "outside":
        for group in (dense, hashed):
            assert any(bool((signed(lv[l].cell) < 0).any()) for l in group) and any(bool((signed(lv[l].cell) > lv[l].res - 1).any()) for l in group)
        assert not inside
    else:
        raise KeyError(which)
