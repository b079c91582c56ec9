"""The exact reference of the hash-grid forward (tests/hashgrid_forward_reference.py) against exact rational arithmetic, its own limit,
the float64 oracle and hand-worked hash indices; the conditions that the inputs of tests/test_hashgrid_forward_exact_gpu.py must meet;
and five wrong kernels, each restated as a mutation of the emulation, that the GPU test's check must refuse -- all without a GPU."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import tcnn_oracle as T
from tests import hashgrid_forward_cases as H
from tests import hashgrid_forward_reference as F
from tests import kat_independent as KAT
from tests import table_backward_reference as R


# ---- fma_f32 with a general addend -----------------------------------------------------------------------------------------------------
def round_once_to_f32(q):
    """A Fraction rounded to the nearest normal f32, ties to even, by integer arithmetic alone."""
    if q == 0:
        return 0.0
    sign, a = (-1.0 if q < 0 else 1.0), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length() - 24
    while a / Fraction(2) ** e >= 1 << 24:
        e += 1
    while a / Fraction(2) ** e < 1 << 23:
        e -= 1
    m = a / Fraction(2) ** e                                          # in [2^23, 2^24)
    k = m.numerator // m.denominator
    rest = m - k
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and k & 1):
        k += 1
    assert -126 <= e + 23 <= 127
    return sign * math.ldexp(k, e)


def fma_triples():
    rng = np.random.RandomState(1)
    n = 3000
    mant = lambda m: (1.0 + rng.randint(0, 1 << 23, m) * 2.0 ** -23) * np.where(rng.rand(m) < 0.5, -1.0, 1.0)
    a = np.ldexp(mant(n), rng.randint(-20, 20, n))
    b = np.ldexp(mant(n), rng.randint(-20, 20, n))
    # addends from 2^70 above the product (the product is far below one f64 spacing of the sum) to far below it
    c = np.ldexp(mant(n), np.frexp(a * b)[1] + rng.randint(-30, 71, n))
    c[::50] = 0.0
    # exact f32 midpoints: the product is half a spacing of the addend, to either side
    m = 400
    c2 = np.ldexp(mant(m), rng.randint(-10, 10, m))
    half = np.ldexp(1.0, np.frexp(np.abs(c2))[1] - 1 - 24)
    a2, b2 = half * np.where(rng.rand(m) < 0.5, -1.0, 1.0), np.ones(m)
    # a hair off the midpoint, by less than one f64 spacing of the sum: only the dropped part tells which way the fma rounds.
    # p = (2^12 +- 2^-11)(2^12 + 2^-11) = 2^24 {- 2^-22 | + 2^-10 + 2^-22}; the addend's spacing is 2^25, its midpoints are c + 2^24
    a3 = np.array([2.0 ** 12 - 2.0 ** -11, 2.0 ** 12 + 2.0 ** -11] * 2)
    b3 = np.full(4, 2.0 ** 12 + 2.0 ** -11)
    c3 = np.array([(2 ** 23 + 1) * 2.0 ** 25, (2 ** 23 + 2) * 2.0 ** 25, -(2 ** 23 + 2) * 2.0 ** 25 - 2.0 ** 25, (2 ** 23 + 5) * 2.0 ** 25])
    cat = lambda *xs: np.concatenate(xs).astype(np.float32)
    return cat(a, a2, a3), cat(b, b2, b3), cat(c, c2, c3)


def test_fma_with_a_general_addend_is_the_exact_sum_rounded_once():
    a, b, c = fma_triples()
    assert a.size > 3000 and np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(c).all()
    got = F.fma_f32(a, b, c)
    want = np.array([round_once_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    # the cases are what they claim to be: products below half an f64 spacing of the sum, exact ties, and results that the naive
    # "round the f64 sum" gets wrong (so the test tells the two apart)
    p, c64 = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    assert ((p != 0) & (c64 != 0) & (np.abs(p) < np.abs(c64) * 2.0 ** -54)).sum() > 300
    naive = (p + c64).astype(np.float32)
    assert (naive != want).any()
    s = slice(3000, 3400)
    exact = [Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)) for x, y, z in zip(a[s], b[s], c[s])]
    ties = sum(any(q == (Fraction(float(w)) + Fraction(float(v))) / 2 for v in (np.nextafter(w, np.float32(-np.inf)), np.nextafter(w, np.float32(np.inf))))
               for q, w in zip(exact, want[s]))
    assert ties > 300                                                # (the rest: the addend's neighbour is a power of two away)
    with pytest.raises(ValueError):
        F.fma_f32(np.float32([2.0 ** -70]), np.float32([2.0 ** -70]), np.float32([0.0]))      # a subnormal result: refused, not guessed


# ---- the limit holds for the kernel's operation order ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", H.GRID_NAMES)
def test_emulation_lies_within_the_limit_of_the_exact_value(name):
    """If the derived limit were tighter than 11 roundings in this order allow, the emulation would leave it somewhere here."""
    worst, n, same = 0.0, 0, 0
    for box in H.BOX_NAMES:
        for which in H.SET_NAMES:
            for table in H.TABLE_NAMES:
                ref = H.reference_of(name, box, which, table)
                bad, what, ratio = F.out_of_limit(ref.emulated, ref)
                assert bad == 0, (name, box, which, table, what)
                worst = max(worst, ratio)
                n += ref.emulated.size
                same += int((ref.emulated.view(np.int16) == ref.exact.astype(np.float16).view(np.int16)).sum())
                if table == "log":
                    out = np.abs(ref.emulated.astype(np.float64))
                    assert np.isfinite(out).all() and out.max() < 40000.0
    print("\n%s: %d outputs, worst error/limit %.4f, %.3f %% equal f16(exact)" % (name, n, worst, 100.0 * same / n))
    assert 0.5 < worst <= 1.0                                         # and the limit is not idly wide either


def test_log_table_gives_subnormal_outputs_and_cancellation():
    ref = H.reference_of("product", "sym", "march", "log")
    out = np.abs(ref.emulated.astype(np.float64))
    assert ((out > 0) & (out < 2.0 ** -14)).any()                      # f16 subnormals
    assert (np.abs(ref.exact) < 1e-3 * ref.mass).any()                # a sum a thousand times below its terms
    t = H.table_of("product", "log").astype(np.float64)
    assert np.abs(t).min() == 2.0 ** -24 and np.abs(t).max() == 30000.0 and (t > 0).any() and (t < 0).any()


# ---- against the float64 oracle, and the cells the oracle gets wrong --------------------------------------------------------------------
def oracle_meta(name):
    grid = H.grid_of(name)[0]
    n_levels, log2_size, base, b, _ = H.GRIDS["product" if name == H.EXACT else name]
    om = T.GridMeta(n_levels, 2, log2_size, base, b)
    om.scale, om.resolution, om.offset, om.total = list(grid.scale), list(grid.resolution), list(grid.offset), grid.offset[-1]
    return om


@pytest.mark.parametrize("name", ["product", "small", H.EXACT])
def test_exact_agrees_with_the_float64_oracle_where_the_cells_agree(name):
    """oracle.tcnn_oracle.hash_encode forms pos = f32(f32(x01 * scale) + 0.5): two roundings, the kernel's fmaf has one.  Where both
    give the same cell (and, on a dense level, a cell inside the grid: the oracle takes a full `%` there, the kernel clamps),

        |exact - oracle| <= (3 u + 3 u^2 + u^3) * sum_c |v_c| + gamma_4 * mass,      u = ulp32(max(|pos|, |pos_oracle|)) per sample

    the two positions differ by at most one ulp per axis (tests/test_table_backward_reference_cpu.py has the argument), a weight is a
    product of three factors in [0, 1] that move by at most u each; the oracle's weights carry 3 f32 roundings and its f64 sums a few
    2^-53.  Where the cells differ the oracle cannot say anything: those (sample, level, axis) triples are counted and printed, and the
    face set must hold some -- this is the gap that only the exact cell closes."""
    grid = H.grid_of(name)[0]
    om = oracle_meta(name)
    table = H.table_of(name, "uniform")
    t64 = torch.from_numpy(table.astype(np.float64))
    differ = {}
    for box in H.BOX_NAMES:
        mn, mx = H.box_of(grid, box)
        for which in ("faces", "march", "corners", "outside"):
            ref = H.reference_of(name, box, which, "uniform")
            x01 = R.unit_positions(H.points_of(name, box, which), mn, mx)
            want = T.hash_encode(torch.from_numpy(x01), t64, om, value_dtype=torch.float64).numpy().reshape(ref.n, grid.n_levels, 2)
            compared = 0
            for l, lv in enumerate(ref.levels):
                pos_o = (x01 * np.float32(lv.scale) + np.float32(0.5)).astype(np.float32)
                cell_o = np.floor(pos_o).astype(np.int64).astype(np.uint32)
                differ[which] = differ.get(which, 0) + int((cell_o != lv.cell).sum())
                ok = (cell_o == lv.cell).all(axis=1)
                if not lv.hashed:
                    ok &= (H.signed(lv.cell) >= 0).all(axis=1) & (H.signed(lv.cell) <= lv.res - 1).all(axis=1)
                u = R.ulp32(np.maximum(np.abs(lv.pos), np.abs(pos_o)).max(axis=1).astype(np.float64))
                tol = ((3 * u + 3 * u * u + u ** 3)[:, None] * np.abs(lv.v.astype(np.float64)).sum(axis=0) + F.gamma(4) * lv.mass)
                err = np.abs(lv.exact - want[:, l])
                assert (err[ok] <= tol[ok]).all(), (name, box, which, l, float((err[ok] / tol[ok]).max()))
                compared += int(ok.sum())
            assert compared > 0.5 * ref.n * grid.n_levels
    print("\n%s: (sample, level, axis) triples whose cell differs between fmaf and two roundings: %r" % (name, differ))
    assert differ["faces"] >= 1                                       # the gap the oracle cannot see
    assert differ["corners"] == 0


def test_corner_indices_reproduce_the_hand_worked_hashes():
    """tests/kat_independent.py HASH_KAT: level 15 of the recipe grid (2^19 entries), through forward_level from POSITIONS -- the
    cells above the grid (12345) are reached from outside the box, as the kernel reaches them."""
    grid = H.grid_of("product")[0]
    l, s = 15, np.float64(np.float32(grid.scale[15]))
    assert grid.offset[16] - grid.offset[15] == 1 << 19
    cells = np.array([c for c, _ in KAT.HASH_KAT], np.float64)
    x = ((cells + 0.25 - 0.5) / s - 0.5).astype(np.float32)           # pos = cell + 0.25
    lv = F.forward_level(x, np.full(3, -0.5, np.float32), np.full(3, 0.5, np.float32), H.table_of("product", "uniform"), grid.resolution[l],
                         grid.offset[l], 1 << 19, grid.scale[l])
    assert np.array_equal(lv.cell, cells.astype(np.uint32)) and lv.hashed
    assert lv.idx[0].tolist() == [want for _, want in KAT.HASH_KAT]
    lv0 = F.forward_level(x[:1], np.full(3, -0.5, np.float32), np.full(3, 0.5, np.float32), H.table_of("product", "uniform"), grid.resolution[l],
                          grid.offset[l], 1 << 19, grid.scale[l])
    assert lv0.idx[:, 0].tolist() == [0, 1, 489905, 489905 ^ 1, 153493, 153493 ^ 1, 489905 ^ 153493, 489905 ^ 153493 ^ 1]


def test_dense_levels_clamp_and_hashed_levels_hash_the_wrapped_cell():
    """Outside the box, by hand: level 0 of the recipe grid (res 16, dense) and level 15 (hashed)."""
    grid = H.grid_of("product")[0]
    mn, mx = np.full(3, -0.5, np.float32), np.full(3, 0.5, np.float32)
    table = H.table_of("product", "uniform")
    x = np.array([[-1.0, 0.0, 2.0]], np.float32)                      # x01 = -0.5, 0.5, 2.5
    lv = F.forward_level(x, mn, mx, table, 16, 0, 4096, grid.scale[0])   # scale 15: pos = -7, 8, 38
    assert H.signed(lv.cell).tolist() == [[-7, 8, 38]] and lv.f.tolist() == [[0.0, 0.0, 0.0]]
    assert lv.idx[0, 0] == 15 + 8 * 16 + 15 * 256                      # the negative cell and the cell above both land on res - 1
    assert float(lv.exact[0, 0]) == float(table[15 + 8 * 16 + 15 * 256, 0])
    lv = F.forward_level(x, mn, mx, table, grid.resolution[15], grid.offset[15], 1 << 19, grid.scale[15])
    cx, cy, cz = [int(v) for v in lv.cell[0]]
    assert cx > 1 << 31 and H.signed(lv.cell)[0, 0] < 0
    assert lv.idx[0, 0] == (cx ^ (cy * R.PRIME_Y & 0xFFFFFFFF) ^ (cz * R.PRIME_Z & 0xFFFFFFFF)) & ((1 << 19) - 1)
    with pytest.raises(ValueError):
        F.cells_of(np.array([[3e9, 0, 0]], np.float32), mn, mx, 1.0)   # |pos| >= 2^31
    with pytest.raises(ValueError):
        F.cells_of(x, mn, np.full(3, 1.0, np.float32), 1.0)            # extent 1.5


# ---- the input gradient ------------------------------------------------------------------------------------------------------------------
def test_input_gradient_reference_is_the_derivative_of_exact():
    """Inside a cell `exact` is trilinear in pos, so a central difference of the float64 interpolant over the SAME cell is its derivative
    up to rounding; and the gradient scales with out_scale and 1 / extent per axis."""
    grid = H.grid_of("small")[0]
    table = H.table_of("small", "uniform")
    rng = np.random.RandomState(3)
    n = 64
    d = (rng.randn(grid.n_levels, n, 2) * 0.05).astype(np.float16)
    for box in H.BOX_NAMES:
        mn, mx = H.box_of(grid, box)
        x = H.to_box(rng.rand(n, 3) * 0.9 + 0.05, mn, mx)
        g = F.input_gradient_reference(x, mn, mx, table, d, grid.resolution, grid.offset, grid.scale, grid.n_levels, 4.0)
        inv = 1.0 / (mx - mn).astype(np.float64)
        num = np.zeros((n, 3))
        for l in range(grid.n_levels):
            lv = F.forward_level(x, mn, mx, table, grid.resolution[l], grid.offset[l], grid.offset[l + 1] - grid.offset[l], grid.scale[l])
            v = (lv.v.astype(np.float64) * d[l].astype(np.float64)[None]).sum(axis=2)       # (8, n)
            f = lv.f.astype(np.float64)
            for k in range(3):
                hi, lo = f.copy(), f.copy()
                hi[:, k], lo[:, k] = 1.0, 0.0                                               # the cell's two faces along k: trilinear, so exact
                num[:, k] += 4.0 * lv.scale * inv[k] * ((F.exact_weights(hi) - F.exact_weights(lo)) * v).sum(axis=0)
        assert np.allclose(g.grad, num, rtol=1e-12, atol=1e-12 * g.mass.max())
        assert (g.mass >= np.abs(g.grad) * (1 - 1e-12)).all() and (g.limit == F.gamma(32) * g.mass).all()
        g1 = F.input_gradient_reference(x, mn, mx, table, d, grid.resolution, grid.offset, grid.scale, grid.n_levels, 1.0)
        assert np.array_equal(g1.grad * 4.0, g.grad)


# ---- the inputs of the GPU tests reach what they are meant to reach --------------------------------------------------------------------
@pytest.mark.parametrize("name", H.GRID_NAMES)
def test_every_condition_of_the_cases_holds(name):
    grid = H.grid_of(name)[0]
    for box in H.BOX_NAMES:
        for which in H.SET_NAMES:
            H.check_conditions(name, box, which)
            assert H.points_of(name, box, which).shape[0] <= 4100
    if name == "levels12":
        assert grid.n_levels == 12 and sum(s * 4 > 1 << 20 for s in H.level_sizes(grid)) >= 2
    if name == "levels4":
        assert grid.n_levels == 4 and grid.resolution[1] ** 3 == H.level_sizes(grid)[1]     # a dense level that fills its table exactly
    if name == H.EXACT:
        assert [grid.resolution[l] for l in (5, 10, 15)] == [64, 256, 1024]
    mn, mx = H.SKEW
    assert len(set((mx - mn).tolist())) == 3 and len(set(mn.tolist())) == 3                # a swapped axis changes the box


def test_counts_cover_the_wave_and_chunk_edges():
    ref = H.reference_of("product", "sym", "march", "uniform")
    counts = H.counts_of(ref)
    assert set(H.COUNTS) <= set(counts) and len(counts) == len(H.COUNTS) + 2 and max(counts) <= ref.n
    assert {H.WAVE - 1, H.WAVE, H.WAVE + 1, H.CHUNK - 1, H.CHUNK, H.CHUNK + 1} <= set(counts) and min(counts) == 1


def test_workgroup_map_of_twelve_levels_covers_every_chunk_once():
    """ngp_debug_hashgrid_fwd_map (host code) on the 12-level grid: every (level, chunk) goes to exactly one workgroup, a level with a
    table above 1 MiB stays on one XCD.  tests/test_capi_cpu.py holds the same for 16 levels."""
    from ngp_pl_amd import _lib
    grid, meta = H.grid_of("levels12")
    for n_chunks in range(1, 41):
        buf = np.full((12 * n_chunks + 8, 3), -1, np.int32)
        n = _lib.call("ngp_debug_hashgrid_fwd_map", C.byref(meta), n_chunks, buf.ctypes.data, buf.shape[0])
        assert n == 12 * n_chunks, (n_chunks, n)
        got = buf[:n]
        assert (buf[n:] == -1).all() and got[:, 0].min() >= 0 and got[:, 0].max() <= 7
        keys = got[:, 1].astype(np.int64) * (1 << 20) + got[:, 2]
        assert len(np.unique(keys)) == n and got[:, 2].min() == 0 and got[:, 2].max() == n_chunks - 1
        assert got[:, 1].min() == 0 and got[:, 1].max() == 11
        for l in range(12):
            assert (got[:, 1] == l).sum() == n_chunks
            if H.level_sizes(grid)[l] * 4 > 1 << 20:
                assert len(np.unique(got[got[:, 1] == l, 0])) == 1, l


# ---- five wrong kernels, as mutations of the emulation: the GPU test's check (F.out_of_limit) must refuse each ----------------------------
def wave_sources(cell, ignore_axis=None):
    """What a kernel that gathers once per run of equal cells inside a wave does: first[i] (sample i gathers), src[i] (the sample whose
    gathered corners sample i uses)."""
    n = cell.shape[0]
    keep = [k for k in range(3) if k != ignore_axis]
    first = np.ones(n, bool)
    first[1:] = (cell[1:, keep] != cell[:-1, keep]).any(axis=1)
    first[::H.WAVE] = True
    src = np.maximum.accumulate(np.where(first, np.arange(n), 0))
    return first, src


def emulate_with(ref, per_level):
    """The emulation with the corner VALUES replaced per level by per_level(lv) -> (8, n, 2) f16 (weights stay the sample's own)."""
    return np.stack([F.emulate(lv.f, per_level(lv)) for lv in ref.levels])


def test_an_off_by_one_in_src_is_refused():
    ref = H.reference_of("product", "sym", "march", "uniform")

    def values(lv):
        first, src = wave_sources(lv.cell)
        take = np.where(src % H.WAVE == 0, src, src - 1)               # one lane too low (lane 0 has no lower lane)
        v = lv.v[:, take].copy()
        v[:, ~first[take]] = 0                                         # a lane that did not gather holds zeros
        return v
    same = emulate_with(ref, lambda lv: lv.v[:, wave_sources(lv.cell)[1]])
    assert np.array_equal(same.view(np.int16), ref.emulated.view(np.int16))                 # the harness itself changes nothing
    assert F.out_of_limit(emulate_with(ref, values), ref)[0] > 1000


def test_a_first_that_ignores_one_coordinate_is_refused():
    for axis in range(3):
        ref = H.reference_of("product", "skew", "axes", "uniform")
        got = emulate_with(ref, lambda lv: lv.v[:, wave_sources(lv.cell, ignore_axis=axis)[1]])
        bad_rows = (np.abs(got.astype(np.float64) - ref.exact) > ref.limit).any(axis=(0, 2))
        assert bad_rows[200 * axis:200 * (axis + 1)].sum() > 50 and F.out_of_limit(got, ref)[0] > 100
        # the march-like rays see it as well
        ref = H.reference_of("product", "sym", "march", "uniform")
        assert F.out_of_limit(emulate_with(ref, lambda lv: lv.v[:, wave_sources(lv.cell, ignore_axis=axis)[1]]), ref)[0] > 100


def two_rounding_forward(name, box, which, table):
    """The forward with pos = f32(f32(x01 * scale) + 0.5) instead of one fmaf, everything else as the emulation."""
    grid = H.grid_of(name)[0]
    mn, mx = H.box_of(grid, box)
    x01 = R.unit_positions(H.points_of(name, box, which), mn, mx)
    t = H.table_of(name, table)
    out, moved = [], 0
    for l in range(grid.n_levels):
        pos = ((x01 * np.float32(grid.scale[l])).astype(np.float32) + np.float32(0.5)).astype(np.float32)
        cell, f = F.cell_from_pos(pos)
        size = grid.offset[l + 1] - grid.offset[l]
        idx = R.corner_indices(cell, grid.resolution[l], size, R.is_hashed(grid.resolution[l], size))
        out.append(F.emulate(f, t[grid.offset[l] + idx]))
        moved += int((pos != F.cells_of(H.points_of(name, box, which), mn, mx, grid.scale[l])[0]).sum())
    return np.stack(out), moved


def test_a_missing_fmaf_is_refused():
    """Two roundings in pos move it by at most one ulp, and across a face the interpolant is continuous: the outputs move by
    ulp32(pos) * slope.  That passes the limit where pos is small; it does not on the fine levels of the scale-16 recipe (pos up to
    2^15, ulp 2^-9 against f16 half-spacings of 2^-12 .. 2^-13), on the face set, which holds the positions where the two differ."""
    bad, moved = 0, 0
    for box in H.BOX_NAMES:
        ref = H.reference_of("scale16", box, "faces", "uniform")
        got, m = two_rounding_forward("scale16", box, "faces", "uniform")
        bad += F.out_of_limit(got, ref)[0]
        moved += m
        assert (got.view(np.int16) != ref.emulated.view(np.int16)).any()                    # and the bit-equality figure sees it on either box
    print("\nmissing fmaf: %d positions differ, %d outputs out of limit" % (moved, bad))
    assert moved >= 1 and bad >= 1


def test_a_dropped_border_clamp_is_refused():
    for name in ("product", "levels4"):
        grid = H.grid_of(name)[0]
        ref = H.reference_of(name, "sym", "outside", "uniform")
        table = H.table_of(name, "uniform")

        def values(lv):
            if lv.hashed:
                return lv.v
            c = lv.cell.astype(np.uint64)
            base = (c[:, 0] + c[:, 1] * np.uint64(lv.res) + c[:, 2] * np.uint64(lv.res * lv.res)) & np.uint64(0xFFFFFFFF)
            idx = np.stack([(base + np.uint64((k & 1) + ((k >> 1) & 1) * lv.res + (k >> 2) * lv.res * lv.res)) & np.uint64(0xFFFFFFFF) for k in range(8)])
            return table[lv.offset + (idx % np.uint64(lv.size)).astype(np.int64)]            # (a real kernel would read out of bounds)
        got = emulate_with(ref, values)
        bad = np.abs(got.astype(np.float64) - ref.exact) > ref.limit
        assert bad[H.dense_levels(grid)].sum() > 100 and not bad[H.hashed_levels(grid)].any()
        assert F.out_of_limit(got, ref)[0] == bad.sum()


def test_an_unwritten_tail_chunk_is_refused():
    ref = H.reference_of("product", "sym", "march", "uniform")
    for n in (257, 1023, 4097):
        rows = np.arange(n)
        got = ref.emulated[:, :n].copy()
        assert F.out_of_limit(got, ref, rows)[0] == 0
        got[:, (n - 1) // H.CHUNK * H.CHUNK:] = np.float16(np.nan)      # the prefill of the GPU test's output buffer
        assert F.out_of_limit(got, ref, rows)[0] == ((n - 1) % H.CHUNK + 1) * 2 * ref.n_levels
