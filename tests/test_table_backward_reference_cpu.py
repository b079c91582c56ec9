"""The exact integer reference of the table backward (tests/table_backward_reference.py) against float64 autograd of the oracle,
its own invariants, and the conditions that the inputs of tests/test_table_backward_exact_gpu.py must meet -- all without a GPU."""
import numpy as np
import pytest
import torch

from oracle import tcnn_oracle as T
from tests import table_backward_cases as K
from tests import table_backward_reference as R

SMALL_N = (0, 1, 63, 1023, 1024, 1025, 3079)


def test_reference_against_float64_autograd_of_the_oracle():
    """Per entry and feature:  |Q * 2^-24 - want64| <= n_e * 2^-25 + 3 * ulp32(scale_l + 1) * sum |g|.

    want64 = sum of w_o * g in f64, w_o the oracle's f32 corner weights.  Q * 2^-24 = sum of rint(f32(w * g) * 2^24) * 2^-24.
      * n_e * 2^-25: every term is rounded to a multiple of 2^-24.
      * positions: the oracle forms pos = f32(f32(x01 * scale) + 0.5), the reference fmaf(x01, scale, 0.5).  Below 2^23 adding 0.5 to an
        f32 is exact (or rounds by a quarter of the larger binade's ulp where the sum crosses a power of two), so the oracle is off the
        exact position by at most ulp/2 .. ulp/4 + ulp/4, the fma by ulp/2: the two differ by at most one ulp u = ulp32(scale + 1) per
        axis (every pos is below scale + 1).  A corner weight is a product of three hat functions of slope 1 whose other two
        factors are at most 1, so it moves by at most 3 u; across a cell face the hat functions are continuous, but the sample then
        reaches entries of the NEIGHBOUR cell too: sum |g| runs over the samples that reach the entry in either evaluation.
      * not in the bound, and all far below u >= 2^-19: the f32 roundings inside the weights (5 * 2^-25 on each side), the f32
        rounding of w * g (2^-24 |g|), second order in u (3 u^2), f64 summation.  The worst case 3 u needs a sample ON a lattice
        point with all three positions a full ulp apart; the slack that leaves is what these terms use.  The figure is printed."""
    grid, meta = K.native_grid("product")
    om = T.GridMeta(16, 2, 19, 16, K.GRIDS["product"][3])
    assert om.resolution == grid.resolution and om.offset == grid.offset and om.scale == grid.scale
    n = 4096
    x = K.make_points(n, grid.half, seed=11)
    d = K.make_seeds(n, grid.n_levels, seed=12)
    ref = K.reference_of(grid, x, d)
    x01 = R.unit_positions(x.numpy(), grid.xyz_min, grid.xyz_max)
    table = torch.zeros(om.total, 2, dtype=torch.float64, requires_grad=True)
    out = T.hash_encode(torch.from_numpy(x01), table, om, value_dtype=torch.float64)
    out.backward(d.permute(1, 0, 2).reshape(n, 32).double())
    want = table.grad.numpy()
    sum_g = np.zeros((om.total, 2))
    u = np.zeros(om.total)
    moved = 0
    for l, lv in enumerate(ref.levels):
        a = np.abs(d[l].numpy().astype(np.float64))[lv.j]
        for c in range(8):
            for k in range(2):
                np.add.at(sum_g[:, k], lv.offset + lv.idx[c], a[:, k])
        # the oracle's own cell, where its two roundings put the sample across a face
        s = np.float32(grid.scale[l])
        pos_o = (x01[lv.j] * s + np.float32(0.5)).astype(np.float32)
        cell_o = np.floor(pos_o).astype(np.int64).astype(np.uint32)
        other = (cell_o != lv.cell).any(axis=1)
        moved += int(other.sum())
        if other.any():
            idx_o = R.corner_indices(cell_o[other], lv.res, lv.size, lv.hashed)
            for c in range(8):
                for k in range(2):
                    np.add.at(sum_g[:, k], lv.offset + idx_o[c], a[other][:, k])
        u[lv.offset:lv.offset + lv.size] = R.ulp32(grid.scale[l] + 1.0)
    err = np.abs(ref.Q.astype(np.float64) / R.FIX_ONE - want)        # |Q| < 2^53: exact in f64
    bound = ref.n_e[:, None] * 2.0 ** -25 + 3.0 * u[:, None] * sum_g
    touched = sum_g > 0
    ratio = float((err[touched] / bound[touched]).max())
    print("\nreference vs f64 autograd: worst error / bound %.3f, %d samples in another cell for the oracle, %d entries touched" % (
        ratio, moved, int(touched.sum())))
    assert (err <= bound).all(), ratio
    assert not want[~touched].any() and not ref.Q[~touched].any()
    assert touched.sum() > 100000


def test_permuting_the_samples_leaves_every_sum_identical():
    c = K.plain_case("small", 3079)
    perm = torch.randperm(3079, generator=torch.Generator().manual_seed(5))
    again = K.reference_of(c.grid, c.x[perm], c.d[:, perm])
    assert np.array_equal(again.Q, c.ref.Q) and np.array_equal(again.n_e, c.ref.n_e) and np.array_equal(again.M_e, c.ref.M_e)


def test_a_levels_entries_sum_to_the_levels_terms():
    c = K.plain_case("small", 3079)
    for lv in c.ref.levels:
        assert np.array_equal(c.ref.Q[lv.offset:lv.offset + lv.size].sum(axis=0), lv.q.sum(axis=(0, 1)))
        assert int(c.ref.n_e[lv.offset:lv.offset + lv.size].sum()) == 8 * lv.j.size


def test_two_halves_add_up_to_the_whole():
    c = K.plain_case("small", 3079)
    h = 1500
    a = K.reference_of(c.grid, c.x[:h], c.d[:, :h])
    b = K.reference_of(c.grid, c.x[h:], c.d[:, h:].contiguous())
    assert np.array_equal(a.Q + b.Q, c.ref.Q) and np.array_equal(a.n_e + b.n_e, c.ref.n_e)


def test_live_prefix_and_indirection_select_the_same_terms():
    c = K.plain_case("small", 3079)
    m = 1300
    act = K.make_active(3079, m, seed=6)
    d = torch.zeros_like(c.d)
    d[:, :m] = c.d[:, act.long()]
    d[:, m:] = 7.0                                                     # columns past the live prefix are never read
    got = K.reference_of(c.grid, c.x, d, torch.cat([act, torch.full((3079 - m,), -1, dtype=torch.int32)]), m)
    want = K.reference_of(c.grid, c.x[act.long()], c.d[:, act.long()].contiguous())
    assert np.array_equal(got.Q, want.Q)
    assert not K.reference_of(c.grid, c.x, d, None, 0).Q.any()
    assert np.array_equal(K.reference_of(c.grid, c.x, c.d, None, 3079 + 5).Q, c.ref.Q)      # clamped to the batch


def test_write_out_rounds_twice_to_nearest_even_and_saturates():
    q = np.array([[0, 1], [(1 << 24) + 1, -(1 << 24)], [65504 << 24, (65520 << 24)], [-(70000 << 24), (1 << 13) + 1],
                  [(1 << 25) + 1, (1 << 40) + (1 << 16)]], np.int64)
    got = R.write_out(q).astype(np.float64)
    # 2^25 + 1 units round to 2^25 in f32 (first rounding); 2^40 + 2^16 units = 65536 + 2^-8 saturates
    assert got.tolist() == [[0.0, 2.0 ** -24], [1.0, -1.0], [65504.0, 65504.0], [-65504.0, 2.0 ** -11], [2.0, 65504.0]]
    assert R.ulp16(np.array([0.0, 2.0 ** -24, 1.0, 1.5, 65504.0])).tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 32.0]
    with pytest.raises(ValueError):
        R.unit_positions(np.zeros((1, 3), np.float32), [-0.5] * 3, [1.0] * 3)          # extent 1.5: out of the reference's scope


# ---- the inputs of the GPU tests reach what they are meant to reach ---------------------------------------------------------------
def test_small_grid_has_every_dense_split_and_a_partial_last_slice():
    grid, _ = K.native_grid("small")
    assert grid.n_levels < 16 and K.GRIDS["small"][1] in (14, 15)
    assert K.dense_split_branches(grid) == (True, True, True), (grid.resolution, K.level_sizes(grid))
    assert K.has_partial_last_slice(grid)
    assert len(K.dense_levels(grid)) < grid.n_levels


@pytest.mark.parametrize("name,n", [("small", n) for n in SMALL_N] + [("product", 20011), ("scale16", 20011)])
def test_plain_cases_cover_their_conditions(name, n):
    c = K.plain_case(name, n)
    assert n * c.grid.n_levels * 8 <= 2_600_000
    x01 = R.unit_positions(c.x.numpy(), c.grid.xyz_min, c.grid.xyz_max)
    if n >= 8:
        for axis in range(3):
            assert (x01[:, axis] == 0).any() and (x01[:, axis] == 1).any()       # the closed box, both faces of every axis
    elif n == 1:
        assert (x01 == 1).any() and (x01 == 0).any()
    if n >= 63:
        assert K.seeds_cover_the_range(c.d)
    if name != "small":
        # the pair (x, .), (x + 1, .) differs in the low bits that x + 1 carries through: it can only lie across a multiple of 6912 = 27 * 2^8
        # when x ends in eight one bits, i.e. from resolution 256 up -- the recipe grids have such levels, the small grid cannot
        assert K.straddling_pairs(c.ref) >= 20
    if name == "scale16":
        assert max(c.grid.scale) > 2 ** 15 - 2 and float(c.x.abs().max()) == 16.0


def test_crowd_cases_cover_their_conditions():
    for big in (False, True):
        c = K.crowd_case("small", 4096, big)
        assert K.max_contributions_of_one_block(c.ref) > 512
        assert K.dense_levels_hold_one_cell(c.ref)
        fine = c.ref.levels[-1]
        assert fine.hashed and bool((fine.cell == fine.cell[0]).all())
    exact = c.ref.Q.astype(np.float64) / R.FIX_ONE                    # (the +60 000 case)
    over = exact > R.F16_MAX
    assert over.any() and (c.ref.f16_exact[over] == np.float16(65504.0)).all() and np.isfinite(c.ref.f16_exact.astype(np.float32)).all()
    for l in K.dense_levels(c.grid):                                  # saturation is reached on the K-split levels and on the hashed ones
        assert over[c.grid.offset[l]:c.grid.offset[l + 1]].any()
    assert over[c.grid.offset[c.grid.n_levels - 1]:].any()
