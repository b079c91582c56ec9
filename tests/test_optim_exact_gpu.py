"""The optimizer, loss and AMP kernels of csrc/optim.hip against tests/optim_reference.py: float64 restatements with derived
bounds (Adam, loss seeds, blend, the partial-sum reductions) and exact expectations (casts, slice sums, the non-finite check,
the overwrite-mode loss reduction).  No element is left out of a comparison, and no tolerance here is fitted to the device except
the two logarithm errors R.TAU_FAST / R.TAU_LOGF, which test_device_logarithms_stay_inside_tau measures again on every run.
tests/test_optim_reference_cpu.py proves the reference and its bounds on the same cases without a GPU.

Each Adam test prints the largest fraction of (e_p, e_m, e_v) the device reached.  On an MI355X: 0.50, 0.64 and 0.60 (the dense
update over 4.2 M elements), against 0.50, 0.61 and 0.66 for uncontracted numpy float32 on the CPU.  The logarithms measured 2.925
(`__logf`) and 2.862 (`logf`) units of E max(1, |log x|); both tolerances are 16.

Each of these changes to the kernels, made one at a time in a scratch build, fails the tests named: the sign of adam_one's weight
decay term, bc1 in place of bc2, a scalar tail one element short (the dense, field, merge and shard tests); the sign of
adam_from_partials' weight decay term, its second accumulator dropped (the partials, field, merge and shard tests); 1 / n for
1 / (3 n) in the colour seed (test_nerf_loss, the ticket test); the halfword parity of the float32 tail of the non-finite check
(both found_inf tests, f32); the overwrite-mode threshold at 256 x 63 rays (test_overwrite_mode_adds_the_workgroups_in_order)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import optim_reference as R

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from ngp_pl_amd import _lib
    return _lib


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def flag_tensor(value):
    return torch.tensor([value], dtype=torch.int32, device="cuda")


PH_FILL = 7.0


class Block:
    """One parameter block on the device: master, moments and the f16 working copy (pre-filled, so that a missing write shows)."""

    def __init__(self, p, m, v, with_ph=True):
        self.p0, self.m0, self.v0 = p, m, v
        self.p, self.m, self.v = dev(p), dev(m), dev(v)
        self.ph = torch.full((len(p),), PH_FILL, dtype=torch.float16, device="cuda") if with_ph else None

    def ptrs(self, lib):
        """(param, param_h) and (m, v) pointers."""
        return (lib.ptr(self.p), lib.ptr(self.ph)), (lib.ptr(self.m), lib.ptr(self.v))

    def got(self):
        return host(self.p), host(self.m), host(self.v)

    def check_updated(self, alts, what):
        got = self.got()
        assert all(np.isfinite(x).all() for x in got), what
        fr = R.worst_fraction(got, alts)
        assert max(fr) <= 1.0, (what, fr)
        if self.ph is not None:
            with np.errstate(over="ignore"):
                assert same_bits(host(self.ph), got[0].astype(np.float16)), what
        return np.array(fr)

    def check_unchanged(self, what):
        got = self.got()
        assert same_bits(got[0], self.p0) and same_bits(got[1], self.m0) and same_bits(got[2], self.v0), what
        if self.ph is not None:
            assert bool((self.ph == PH_FILL).all()), what


# ------------------------------------------------------------------------------------------------------------------------------
# dense Adam
# ------------------------------------------------------------------------------------------------------------------------------

def dense_step(lib, p, m, v, g, coef, with_ph=True, flag=None):
    blk = Block(p, m, v, with_ph)
    tg = dev(g)
    (pp, ph), (pm, pv) = blk.ptrs(lib)
    lib.call("ngp_adam_step", pp, ph, lib.ptr(tg), int(g.dtype == f32), pm, pv, len(p), *coef.launch_args(), lib.ptr(flag), lib.stream())
    return blk, host(tg)


@pytest.mark.parametrize("grad_is_f32", [False, True], ids=["f16", "f32"])
def test_dense_adam_small_sizes(lib, grad_is_f32):
    """ngp_adam_step at every size around the 4-wide trip and its scalar tail, every step / weight decay / grad scale: p, m, v of
    every element inside the bound, the f16 copy bit-equal to the rounded master, the gradient zeroed.  The f16 path's +-inf and
    NaN gradients act as +-65504 (adam_dense's comment).  An all-zero element with wd = 0 keeps its parameter bit for bit."""
    worst = np.zeros(3)
    for n in R.ADAM_SIZES:
        for t, wd, gs in R.adam_combos():
            p, m, v, g, kind = R.adam_dense_inputs(n, grad_is_f32, gs)
            coef = R.AdamCoef(wd=wd, step=t, grad_scale=gs)
            blk, g_after = dense_step(lib, p, m, v, g, coef)
            worst = np.maximum(worst, blk.check_updated(R.adam_dense_reference(p, m, v, g, coef), (n, t, wd, gs)))
            assert not bits(g_after).any(), (n, t, wd, gs)
            zero = kind == 0
            if wd == 0.0 and zero.any():
                assert same_bits(blk.got()[0][zero], p[zero])
        # param_h = NULL: the same update
        t, wd, gs = 7, 1e-2, 3.0
        p, m, v, g, kind = R.adam_dense_inputs(n, grad_is_f32, gs, seed=1)
        coef = R.AdamCoef(wd=wd, step=t, grad_scale=gs)
        blk, g_after = dense_step(lib, p, m, v, g, coef, with_ph=False)
        blk.check_updated(R.adam_dense_reference(p, m, v, g, coef), (n, "no param_h"))
        with_copy, _ = dense_step(lib, p, m, v, g, coef)
        assert all(same_bits(a, b) for a, b in zip(blk.got(), with_copy.got()))
        # a raised flag: nothing changes, the gradient is still cleared (include/ngp_hip.h: GradScaler semantics)
        blk, g_after = dense_step(lib, p, m, v, g, coef, flag=flag_tensor(1))
        blk.check_unchanged((n, "flag"))
        assert not bits(g_after).any()
        # a flag that is present and 0 does not skip
        blk, _ = dense_step(lib, p, m, v, g, coef, flag=flag_tensor(0))
        assert all(same_bits(a, b) for a, b in zip(blk.got(), with_copy.got()))
    print("adam-bound-fraction dense-small-%s p %.3f m %.3f v %.3f" % (("f32" if grad_is_f32 else "f16",) + tuple(worst)))


@pytest.mark.parametrize("grad_is_f32", [False, True], ids=["f16", "f32"])
def test_dense_adam_second_grid_stride_trip(lib, grad_is_f32):
    """4 194 311 parameters: more than 4096 workgroups x 256 threads x 4, so the loop takes a second trip, and a scalar tail of 3."""
    n, (t, wd, gs) = R.ADAM_LARGE, (1000, 1e-2, 3.0)
    p, m, v, g, kind = R.adam_dense_inputs(n, grad_is_f32, gs)
    coef = R.AdamCoef(wd=wd, step=t, grad_scale=gs)
    blk, g_after = dense_step(lib, p, m, v, g, coef)
    fr = blk.check_updated(R.adam_dense_reference(p, m, v, g, coef), "large")
    assert not bits(g_after).any()
    blk, g_after = dense_step(lib, p, m, v, g, coef, flag=flag_tensor(1))
    blk.check_unchanged("large, flag")
    assert not bits(g_after).any()
    print("adam-bound-fraction dense-large-%s p %.3f m %.3f v %.3f" % (("f32" if grad_is_f32 else "f16",) + tuple(fr)))


# ------------------------------------------------------------------------------------------------------------------------------
# Adam from partial sums
# ------------------------------------------------------------------------------------------------------------------------------

def test_partials_adam(lib):
    """ngp_adam_step_partials for every row count around its 16-row stride and 8-row tail and every column count around a
    32-column workgroup: the float64 column sum as the gradient, its summation bound carried through the update."""
    worst = np.zeros(3)
    for n_partials in R.PARTIALS_ROWS:
        for n in R.PARTIALS_N:
            t, wd, gs = R.partials_combo(n_partials, n)
            p, m, v, rows = R.partials_inputs(n_partials, n)
            coef = R.AdamCoef(wd=wd, step=t, grad_scale=gs)
            alts = [R.adam_partials_reference(p, m, v, rows, coef)]
            trows = dev(rows) if n_partials else None
            for flag in (None, 1):
                blk = Block(p, m, v)
                (pp, ph), (pm, pv) = blk.ptrs(lib)
                tflag = None if flag is None else flag_tensor(flag)
                lib.call("ngp_adam_step_partials", pp, ph, lib.ptr(trows), n_partials, pm, pv, n, *coef.launch_args(),
                         lib.ptr(tflag), lib.stream())
                if flag:
                    blk.check_unchanged((n_partials, n, "flag"))
                else:
                    worst = np.maximum(worst, blk.check_updated(alts, (n_partials, n, t, wd, gs)))
            if n_partials:
                assert same_bits(host(trows), rows)                     # the partial sums are read only
    assert any(R.partials_combo(a, b)[1] > 0 for a in R.PARTIALS_ROWS for b in R.PARTIALS_N)
    print("adam-bound-fraction partials p %.3f m %.3f v %.3f" % tuple(worst))


# ------------------------------------------------------------------------------------------------------------------------------
# the field launches
# ------------------------------------------------------------------------------------------------------------------------------

N_DENSITY, N_RGB, ROWS = 33, 65, 9


def field_blocks(n_grid, seed):
    """Grid block (f16 gradient, scale 128) and the two MLP blocks with their partial rows."""
    p, m, v, g, _ = R.adam_dense_inputs(n_grid, False, 128.0, seed=seed)
    g = np.where(np.isfinite(g), g, np.float16(12.5)).astype(np.float16)         # (the non-finite specials belong to the dense test)
    grid = (p, m, v, g)
    dens = R.partials_inputs(ROWS, N_DENSITY, seed=seed)
    rgb = R.partials_inputs(ROWS, N_RGB, seed=seed + 1)
    return grid, dens, rgb


def field_args(lib, gblk, tgrad, n_grid, dblk, drows, rblk, rrows, coef):
    (gp, gph), (gm, gv) = gblk.ptrs(lib)
    (dp, dph), (dm, dv) = dblk.ptrs(lib)
    (rp, rph), (rm, rv) = rblk.ptrs(lib)
    return (gp, gph, lib.ptr(tgrad), gm, gv, n_grid, dp, dph, lib.ptr(drows), dm, dv, N_DENSITY, rp, rph, lib.ptr(rrows), rm, rv, N_RGB,
            ROWS) + coef.launch_args()


@pytest.mark.parametrize("zero_grid_grad", [1, 0])
def test_field_adam(lib, zero_grid_grad):
    """ngp_adam_step_field: the grid block and both MLP blocks of one launch against the reference; the grid gradient zeroed or left
    alone as zero_grid_grad says; under a raised flag nothing changes and the gradient is cleared only if asked."""
    n_grid = 1027
    coef = R.AdamCoef(wd=1e-2, step=2, grad_scale=128.0)
    grid, dens, rgb = field_blocks(n_grid, 3)
    worst = np.zeros(3)
    for flag in (None, 1):
        gblk, dblk, rblk = Block(*grid[:3]), Block(*dens[:3]), Block(*rgb[:3])
        tgrad, drows, rrows = dev(grid[3]), dev(dens[3]), dev(rgb[3])
        tflag = None if flag is None else flag_tensor(flag)
        lib.call("ngp_adam_step_field", *field_args(lib, gblk, tgrad, n_grid, dblk, drows, rblk, rrows, coef), zero_grid_grad,
                 lib.ptr(tflag), None, lib.stream())
        if flag:
            for b in (gblk, dblk, rblk):
                b.check_unchanged("flag")
        else:
            worst = np.maximum(worst, gblk.check_updated(R.adam_dense_reference(*grid, coef), "grid"))
            worst = np.maximum(worst, dblk.check_updated([R.adam_partials_reference(*dens, coef)], "density"))
            worst = np.maximum(worst, rblk.check_updated([R.adam_partials_reference(*rgb, coef)], "rgb"))
        g_after = host(tgrad)
        assert (not bits(g_after).any()) if zero_grid_grad else same_bits(g_after, grid[3])
    print("adam-bound-fraction field p %.3f m %.3f v %.3f" % tuple(worst))


def test_field_adam_merge(lib):
    """ngp_adam_step_field_merge with a hand-made record: 3 levels of 8, 16 and 40 entries split into 1, 2 and 5 partial tables,
    value_end = 128 < n_grid.  Below value_end the gradient is the float32 sum of the parts in part order, saturated and rounded to
    f16 (exact in numpy; some sums leave the f16 range); beyond it the plain f16 gradient.  grid_grad is left untouched -- below
    value_end it is not even read (it holds a poison value)."""
    sizes, k_split = (8, 16, 40), (1, 2, 5)
    offsets = [0, 8, 24, 64]
    part_off, total = [], 0
    for s, k in zip(sizes, k_split):
        part_off.append(total)
        total += s * k
    value_end, n_grid = 2 * offsets[-1], 2 * offsets[-1] + 39
    rng = np.random.default_rng(11)
    partial = (rng.choice([-1.0, 1.0], (total, 2)) * 10.0 ** rng.uniform(-3, 4.6, (total, 2))).astype(f32)
    partial[3] = (7.0e4, -2.0e5)                                    # one part alone beyond the f16 range
    partial[part_off[2]: part_off[2] + 5 * 40: 40] = 3.0e4          # entry 0 of level 2: 5 x 3e4
    partial[part_off[2] + 1: part_off[2] + 1 + 5 * 40: 40] = (-2.9e4, 1.0)
    coef = R.AdamCoef(wd=1e-2, step=2, grad_scale=128.0)
    grid, dens, rgb = field_blocks(n_grid, 5)
    g_merge = R.merge_gradient(partial, offsets, k_split, part_off)
    assert np.count_nonzero(np.abs(g_merge.astype(f64)) == R.F16_MAX) >= 5 and np.isfinite(g_merge).all()
    g_table = grid[3].copy()
    g_table[:value_end] = np.float16(777.0)
    g_eff = np.concatenate([g_merge, grid[3][value_end:]])
    tpart = dev(partial)
    rec = lib.GridPartials()
    rec.n_levels, rec.value_end, rec.partial = 3, value_end, tpart.data_ptr()
    for l in range(3):
        rec.offset[l], rec.k_split[l], rec.part_off[l] = offsets[l], k_split[l], part_off[l]
    rec.offset[3] = offsets[3]
    gblk, dblk, rblk = Block(*grid[:3]), Block(*dens[:3]), Block(*rgb[:3])
    tgrad, drows, rrows = dev(g_table), dev(dens[3]), dev(rgb[3])
    lib.call("ngp_adam_step_field_merge", *field_args(lib, gblk, tgrad, n_grid, dblk, drows, rblk, rrows, coef), None, None,
             C.byref(rec), lib.stream())
    fr = gblk.check_updated(R.adam_dense_reference(grid[0], grid[1], grid[2], g_eff, coef), "grid")
    fr = np.maximum(fr, dblk.check_updated([R.adam_partials_reference(*dens, coef)], "density"))
    fr = np.maximum(fr, rblk.check_updated([R.adam_partials_reference(*rgb, coef)], "rgb"))
    assert same_bits(host(tgrad), g_table) and same_bits(host(tpart), partial)
    print("adam-bound-fraction merge p %.3f m %.3f v %.3f" % tuple(fr))


@pytest.mark.parametrize("skip_mlp", [0, 1])
@pytest.mark.parametrize("skip_grid", [0, 1])
def test_field_adam_shard_flags_decide_their_blocks(lib, skip_mlp, skip_grid):
    """ngp_adam_step_field_shard: found_inf_mlp decides both MLP blocks, found_inf_shard the grid block, independently: a block is
    inside the bound or bit-unchanged.  The gradient is never cleared.  With a step_state the two applied-step counts advance
    independently (exact integers; the bias correction from the device-side count stays with the existing step-count test, so the
    value check runs without a step_state)."""
    n_grid = 1027
    coef = R.AdamCoef(wd=1e-2, step=7, grad_scale=128.0)
    grid, dens, rgb = field_blocks(n_grid, 9)
    for with_state in (False, True):
        gblk, dblk, rblk = Block(*grid[:3]), Block(*dens[:3]), Block(*rgb[:3])
        tgrad, drows, rrows = dev(grid[3]), dev(dens[3]), dev(rgb[3])
        st = torch.tensor([3, -1, 5, -1], dtype=torch.int32, device="cuda") if with_state else None
        args = list(field_args(lib, gblk, tgrad, n_grid, dblk, drows, rblk, rrows, coef))
        if with_state:
            args[-2] = 1                                            # `step` is then the 1-based number of the call: reads slot 0, writes slot 1
        f_mlp, f_grid = flag_tensor(skip_mlp), flag_tensor(skip_grid)
        lib.call("ngp_adam_step_field_shard", *args, lib.ptr(f_mlp), lib.ptr(f_grid), lib.ptr(st), lib.stream())
        if with_state:
            assert host(st).tolist() == [3, 3 + (1 - skip_mlp), 5, 5 + (1 - skip_grid)]
            for b, skipped in ((gblk, skip_grid), (dblk, skip_mlp), (rblk, skip_mlp)):
                if skipped:
                    b.check_unchanged("skipped")
                else:
                    with np.errstate(over="ignore"):
                        assert not same_bits(b.got()[0], b.p0) and same_bits(host(b.ph), b.got()[0].astype(np.float16))
        else:
            if skip_grid:
                gblk.check_unchanged("grid")
            else:
                gblk.check_updated(R.adam_dense_reference(*grid, coef), "grid")
            for b, data in ((dblk, dens), (rblk, rgb)):
                if skip_mlp:
                    b.check_unchanged("mlp")
                else:
                    b.check_updated([R.adam_partials_reference(*data, coef)], "mlp")
        assert same_bits(host(tgrad), grid[3])


# ------------------------------------------------------------------------------------------------------------------------------
# loss seeds, terms, blend
# ------------------------------------------------------------------------------------------------------------------------------

BG = np.array([0.2, 0.7, 1.0], f32)
LAMBDA, SCALE = 1e-3, 128.0


def loss_inputs(n, seed=0):
    """rgb, gt uniform in [0, 1); opacities drawn from R.log_sweep() (the values the logarithm's error was measured on); the first
    rays take the sweep's edge values in order, so that n = 1 meets opacity 0 and larger batches meet all of them."""
    rng = np.random.default_rng(500 + seed + n)
    sweep = R.log_sweep()
    edges = np.concatenate([sweep[:9], [f32(1.0)]])
    o = rng.choice(sweep, n).astype(f32)
    o[:min(n, len(edges))] = edges[:n]
    return rng.random((n, 3), dtype=f32), o, rng.random((n, 3), dtype=f32)


class LossRun:
    def __init__(self, lib, rgb, o, gt, bg, lam, gs, with_sq=True):
        n = len(o)
        self.inputs = [dev(rgb), dev(o), dev(gt), dev(bg)]
        self.loss = torch.full((1,), 123.0, device="cuda")
        self.sq = torch.full((1,), 123.0, device="cuda") if with_sq else None
        self.d_rgb = torch.full((n, 3), 55.0, device="cuda")
        self.d_o = torch.full((n,), 55.0, device="cuda")
        lib.call("ngp_nerf_loss", *(lib.ptr(t) for t in self.inputs), lam, gs, n, lib.ptr(self.loss), lib.ptr(self.sq),
                 lib.ptr(self.d_rgb), lib.ptr(self.d_o), lib.stream())

    def check(self, ref, n, what):
        d_rgb, d_o = host(self.d_rgb).astype(f64), host(self.d_o).astype(f64)
        assert np.all(np.abs(d_rgb - ref["d_rgb"]) <= ref["e_d_rgb"]), what
        assert np.all(np.abs(d_o - ref["d_o"]) <= ref["e_d_o"]), what
        k = R.loss_reduction_k(n)
        assert abs(float(host(self.loss)[0]) - ref["loss"]) <= ref["e_l"] + k * R.E * np.abs(ref["l_ray"]).sum(), what
        if self.sq is not None:
            assert abs(float(host(self.sq)[0]) - ref["sq_err"]) <= ref["e_se"] + k * R.E * ref["se_ray"].sum(), what


def measure_tau(lib):
    """The device logarithms against float64 over R.log_sweep(), in units of E max(1, |log x|): `__logf` through ngp_nerf_loss
    (no background, lambda = 1, grad_scale = 1, 256 rays: d_o = -(lg + 1) / 256, exact apart from one rounded addition), `logf`
    through ngp_nerf_loss_terms_fw (lambda = 1: ent = -(oe logf(oe)), one rounded product)."""
    sweep = R.log_sweep()
    pad = (-len(sweep)) % 256
    o_all = np.concatenate([sweep, np.full(pad, 0.5, f32)])
    oe = (o_all + R.LOSS_EPS).astype(f64)
    zeros = torch.zeros(256, 3, device="cuda")
    fast, slow = [], []
    for k in range(0, len(o_all), 256):
        to = dev(o_all[k:k + 256])
        out = [torch.empty(1, device="cuda"), torch.empty(256, 3, device="cuda"), torch.empty(256, device="cuda")]
        lib.call("ngp_nerf_loss", lib.ptr(zeros), lib.ptr(to), lib.ptr(zeros), None, 1.0, 1.0, 256, lib.ptr(out[0]), None,
                 lib.ptr(out[1]), lib.ptr(out[2]), lib.stream())
        fast.append(-(host(out[2]).astype(f64) * 256.0) - 1.0)
        sq, ent = torch.empty(256, 3, device="cuda"), torch.empty(256, device="cuda")
        lib.call("ngp_nerf_loss_terms_fw", lib.ptr(zeros), lib.ptr(to), lib.ptr(zeros), 1.0, 256, lib.ptr(sq), lib.ptr(ent), lib.stream())
        slow.append(host(ent).astype(f64))
    fast, slow = np.concatenate(fast), -np.concatenate(slow) / oe
    return float(R.tau_units(fast, oe).max()), float(R.tau_units(slow, oe).max())


def test_device_logarithms_stay_inside_tau(lib):
    """The two fitted numbers of this file, measured again: each device logarithm's error stays below the recorded measurement's
    tolerance (4 x measured, rounded up to a power of two), and what is measured below the defect threshold 2^-20 max(1, |log x|)."""
    fast, slow = measure_tau(lib)
    print("log-tau __logf %.3f (tolerance %g)  logf %.3f (tolerance %g)  [units of E max(1, |log x|)]" % (fast, R.TAU_FAST, slow, R.TAU_LOGF))
    assert fast <= R.TAU_FAST and slow <= R.TAU_LOGF and max(R.MEASURED_TAU_FAST, R.MEASURED_TAU_LOGF, fast, slow) <= R.TAU_DEFECT


@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 255, 256, 257, 16383, 16384, 16385])
def test_nerf_loss(lib, n_rays):
    """ngp_nerf_loss with and without a background, with and without sq_err: every seed inside its per-ray bound, loss and sq_err
    (pre-filled with 123: they are overwritten in both reduction modes) against the float64 sums.  16384 is the last overwrite-mode
    size, 16385 the first atomic-mode one."""
    rgb, o, gt = loss_inputs(n_rays)
    for bg in (BG, None):
        ref = R.nerf_loss_ref(rgb, o, gt, bg, LAMBDA, SCALE)
        for with_sq in (True, False):
            LossRun(lib, rgb, o, gt, bg, LAMBDA, SCALE, with_sq).check(ref, n_rays, (n_rays, bg is None, with_sq))


def test_nerf_loss_ticket_wraps_between_launches_of_different_grids(lib):
    """Three launches back to back with 3, 64 and 1 workgroups and no synchronisation between them: the self-resetting ticket
    (atomicInc wrapping at the launch's own workgroup count) must be back at 0 for each."""
    cases = []
    for n in (3 * 256 - 5, 16384, 1):
        rgb, o, gt = loss_inputs(n, seed=3)
        cases.append((n, R.nerf_loss_ref(rgb, o, gt, BG, LAMBDA, SCALE), (rgb, o, gt)))
    for rounds in range(2):
        runs = [LossRun(lib, *data, BG, LAMBDA, SCALE) for _, _, data in cases]
        for (n, ref, _), run in zip(cases, runs):
            run.check(ref, n, (n, rounds))


def _order_case(n, planted):
    rng = np.random.default_rng(n)
    gt = rng.random((n, 3), dtype=f32)
    rgb = rng.random((n, 3), dtype=f32)
    if planted:                                          # one large workgroup partial, the others 0.3 of its ulp
        rgb = gt.copy()
        rgb[0, 0] = gt[0, 0] + f32(300.0)
        rgb[256::256, 1] = gt[256::256, 1] + f32(0.042)
    o = rng.choice(R.log_sweep(), n).astype(f32)
    return rgb, o, gt


@pytest.mark.parametrize("n_rays,planted", [(763, False), (16384, False), (16384, True)])
def test_overwrite_mode_adds_the_workgroups_in_order(lib, n_rays, planted):
    """Up to 16384 rays the reduction is deterministic: wave sums, (s0 + s1) + (s2 + s3) per workgroup, one wave sum over the
    workgroups' partials in workgroup order.  With lambda = 0 and no background every per-ray term is a handful of uncontracted
    float32 operations (nerf_loss_ray), so loss and sq_err are reproduced BIT FOR BIT.  The planted case makes the order visible:
    adding the small partials to the large one in arrival order (atomics) would lose them."""
    rgb, o, gt = _order_case(n_rays, planted)
    diff = rgb - gt                                       # c + 0 * (1 - o) - g
    se = np.zeros(n_rays, f32)
    for k in range(3):
        se = se + diff[:, k] * diff[:, k]
    inv_3r = f32(1) / (f32(3) * f32(n_rays))
    want_loss, parts = R.overwrite_sum_f32(se * inv_3r)
    want_sq, _ = R.overwrite_sum_f32(se)
    if planted:
        serial = parts[0]
        for x in parts[1:]:
            serial = serial + x
        assert serial != want_loss
    run = LossRun(lib, rgb, o, gt, None, 0.0, SCALE)
    again = LossRun(lib, rgb, o, gt, None, 0.0, SCALE)
    assert same_bits(host(run.loss), np.array([want_loss], f32)) and same_bits(host(run.sq), np.array([want_sq], f32))
    assert same_bits(host(again.loss), host(run.loss)) and same_bits(host(again.sq), host(run.sq))


@pytest.mark.parametrize("n_rays", [1, 255, 256, 257])
def test_loss_terms_forward_and_backward(lib, n_rays):
    rgb, o, gt = loss_inputs(n_rays, seed=5)
    t = [dev(rgb), dev(o), dev(gt)]
    sq, ent = torch.full((n_rays, 3), 55.0, device="cuda"), torch.full((n_rays,), 55.0, device="cuda")
    lib.call("ngp_nerf_loss_terms_fw", *(lib.ptr(x) for x in t), LAMBDA, n_rays, lib.ptr(sq), lib.ptr(ent), lib.stream())
    ref = R.loss_terms_ref(rgb, o, gt, LAMBDA)
    assert np.all(np.abs(host(sq).astype(f64) - ref["sq"]) <= ref["e_sq"])
    assert np.all(np.abs(host(ent).astype(f64) - ref["ent"]) <= ref["e_ent"])
    rng = np.random.default_rng(n_rays)
    g_sq_full, g_ent_full = rng.standard_normal((n_rays, 3)).astype(f32), rng.standard_normal(n_rays).astype(f32)
    for sq_scalar in (0, 1):
        for ent_scalar in (0, 1):
            g_sq = np.array([1.0 / (3 * n_rays)], f32) if sq_scalar else g_sq_full
            g_ent = np.array([-0.37], f32) if ent_scalar else g_ent_full
            tg_sq, tg_ent = dev(g_sq), dev(g_ent)
            g_rgb, g_op = torch.full((n_rays, 3), 55.0, device="cuda"), torch.full((n_rays,), 55.0, device="cuda")
            lib.call("ngp_nerf_loss_terms_bw", lib.ptr(tg_sq), sq_scalar, lib.ptr(tg_ent), ent_scalar, *(lib.ptr(x) for x in t), LAMBDA,
                     n_rays, lib.ptr(g_rgb), lib.ptr(g_op), lib.stream())
            ref = R.loss_terms_bw_ref(g_sq[0] if sq_scalar else g_sq, g_ent[0] if ent_scalar else g_ent, rgb, o, gt, LAMBDA)
            assert np.all(np.abs(host(g_rgb).astype(f64) - ref["g_rgb"]) <= ref["e_g_rgb"]), (sq_scalar, ent_scalar)
            assert np.all(np.abs(host(g_op).astype(f64) - ref["g_opacity"]) <= ref["e_g_opacity"]), (sq_scalar, ent_scalar)


@pytest.mark.parametrize("n_rays", [1, 255, 256, 257])
def test_bg_blend_and_its_backward(lib, n_rays):
    rgb, o, gt = loss_inputs(n_rays, seed=7)
    tbg, trgb, to = dev(BG), dev(rgb), dev(o)
    out = torch.full((n_rays, 3), 55.0, device="cuda")
    lib.call("ngp_bg_blend", lib.ptr(trgb), lib.ptr(to), lib.ptr(tbg), n_rays, lib.ptr(out), lib.stream())
    want = R.bg_blend_ref(rgb, o, BG)
    assert np.all(np.abs(host(out).astype(f64) - want) <= R.ulp32(want))
    rng = np.random.default_rng(n_rays)
    g_rgb, g_o = rng.standard_normal((n_rays, 3)).astype(f32), rng.standard_normal(n_rays).astype(f32)
    for g_in in (g_o, None):
        res = torch.full((n_rays,), 55.0, device="cuda")
        tg_rgb, tg_in = dev(g_rgb), dev(g_in)
        lib.call("ngp_bg_blend_bw", lib.ptr(tg_rgb), lib.ptr(tg_in), lib.ptr(tbg), n_rays, lib.ptr(res), lib.stream())
        want, err = R.bg_blend_bw_ref(g_rgb, g_in, BG)
        assert np.all(np.abs(host(res).astype(f64) - want) <= err), g_in is None


# ------------------------------------------------------------------------------------------------------------------------------
# AMP plumbing: exact
# ------------------------------------------------------------------------------------------------------------------------------

def test_cast_f32_to_f16_rounds_every_value_like_ieee(lib):
    """Every finite f16 value, its float32 neighbours, every tie and its neighbours, the overflow and subnormal boundaries, tiled
    past 8192 x 256 elements (a second grid-stride trip): bit-equal to numpy's round-to-nearest-even."""
    x = R.cast_inputs()
    reps = -(-(8192 * 256 + 4097) // len(x))
    x = np.tile(x, reps)
    assert len(x) > 8192 * 256
    out = torch.full((len(x),), PH_FILL, dtype=torch.float16, device="cuda")
    tx = dev(x)
    lib.call("ngp_cast_f32_to_f16", lib.ptr(tx), len(x), lib.ptr(out), lib.stream())
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    assert same_bits(host(out), want)


@pytest.mark.parametrize("scale", [1.0, 1.0 / 128, 1.0 / 3])
def test_cast_f16_to_f32_scales_every_bit_pattern(lib, scale):
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    out = torch.full((65536,), 55.0, device="cuda")
    th = dev(h)
    lib.call("ngp_cast_f16_to_f32", lib.ptr(th), 65536, scale, lib.ptr(out), lib.stream())
    got = host(out)
    with np.errstate(invalid="ignore"):
        want = h.astype(f32) * f32(scale)
    nan = np.isnan(want)
    assert nan.sum() == 2046 and np.isnan(got[nan]).all() and same_bits(got[~nan], want[~nan])


@pytest.mark.parametrize("count", [8, 2056])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_sum_slices_f16(lib, world, count):
    """Every rank of the world: float32 sum in rank order, one rounding to f16 (ties to even; beyond 65504: inf, no saturation),
    the rank's own slot in `stage` (NaN here) ignored."""
    rng = np.random.default_rng(world * 10000 + count)
    slices = (rng.choice([-1.0, 1.0], (world, count)) * 10.0 ** rng.uniform(-4, 3, (world, count))).astype(np.float16)
    if world > 1:
        slices[:, 0] = 0; slices[0, 0], slices[1, 0] = 2048.0, 1.0                  # 2049: tie, to 2048
        slices[:, 1] = 0; slices[0, 1], slices[world - 1, 1] = 1.0, 2050.0          # 2051: tie, to 2052
        slices[:, 2] = 0; slices[0, 2], slices[1, 2] = 40000.0, 40000.0             # beyond the range: inf
        slices[:, 3] = 0; slices[0, 3], slices[world - 1, 3] = -65504.0, -32.0      # -65536: -inf
        slices[:, count - 1] = 0; slices[world - 1, count - 1] = 0.5; slices[0, count - 1] = 1024.0   # 1024.5: tie, to 1024
    for rank in range(world):
        stage = slices.copy()
        stage[rank] = np.nan
        own = slices[rank].copy()
        want = R.sum_slices_ref(own, stage, rank)
        if world > 1:
            assert want[0] == 2048.0 and want[1] == 2052.0 and np.isposinf(want[2]) and np.isneginf(want[3]) and want[count - 1] == 1024.0
        out = torch.full((count,), PH_FILL, dtype=torch.float16, device="cuda")
        town, tstage = dev(own), dev(stage)
        lib.call("ngp_sum_slices_f16", lib.ptr(town), lib.ptr(tstage), world, rank, count, lib.ptr(out), lib.stream())
        assert not np.isnan(want).any() and same_bits(host(out), want), rank


def test_reduce_partials(lib):
    """ngp_reduce_partials and ngp_reduce_partials2 for every row count around the 32-row stride and 8-row tail, column counts
    around a 32-column workgroup: against the float64 column sums, inside (ceil(n_partials / 8) + 10) E sum |x|."""
    dummy = torch.zeros(1, device="cuda")
    for n_partials in R.REDUCE_ROWS:
        for n_a in R.REDUCE_NA:
            ra = R.partials_inputs(n_partials, n_a, seed=2)[3]
            ta = dev(ra) if n_partials else None
            want_a = ra.astype(f64).sum(0) if n_partials else np.zeros(n_a)
            e_a = R.reduce_bound(ra.reshape(n_partials, n_a), 10)
            out = torch.full((n_a + 2,), 55.0, device="cuda")
            lib.call("ngp_reduce_partials", lib.ptr(ta), n_partials, n_a, lib.ptr(out), lib.stream())
            got = host(out).astype(f64)
            assert np.all(np.abs(got[:n_a] - want_a) <= e_a) and np.all(got[n_a:] == 55.0), (n_partials, n_a)
            for n_b in R.REDUCE_NB:
                rb = R.partials_inputs(n_partials, max(n_b, 1), seed=3)[3][:, :n_b]
                tb = dev(rb) if n_partials and n_b else (dummy if n_partials else None)
                want = np.concatenate([want_a, rb.astype(f64).sum(0) if n_partials else np.zeros(n_b)])
                err = np.concatenate([e_a, R.reduce_bound(rb.reshape(n_partials, n_b), 10)])
                out = torch.full((n_a + n_b + 2,), 55.0, device="cuda")
                lib.call("ngp_reduce_partials2", lib.ptr(ta), n_a, lib.ptr(tb), n_b, n_partials, lib.ptr(out), lib.stream())
                got = host(out).astype(f64)
                assert np.all(np.abs(got[:n_a + n_b] - want) <= err) and np.all(got[n_a + n_b:] == 55.0), (n_partials, n_a, n_b)


# ---- the non-finite check ----

BAD16 = (0x7C00, 0xFC00, 0x7E01, 0xFDFF)                     # +inf, -inf, NaNs with payloads
BAD32 = (0x7F800000, 0xFF800000, 0x7FC00001, 0xFF800001)     # (the last: a signalling NaN whose payload is the lowest bit only)
FINITE16 = (0x7BFF, 0xFBFF)                                  # +-65504
# FLT_MAX; a low halfword with all f16 exponent bits set; two f16 infinities side by side; low halfwords that would pass the
# float32 exponent test if the tail looked at the wrong halfword
FINITE32 = (0x7F7FFFFF, 0xFF7FFFFF, 0x00007C00, 0x7C007C00, 0x00007F80, 0x0000FFFF, 0x7F7F7F80)


def found_inf(lib, words, is_f32, flag_before=0, reset=1):
    """words: the buffer as uint16 / uint32 bit patterns.  Returns the flag after the call."""
    t = dev(words.view(np.int32 if is_f32 else np.int16))
    flag = flag_tensor(flag_before)
    lib.call("ngp_found_inf", lib.ptr(t), int(is_f32), len(words), lib.ptr(flag), reset, lib.stream())
    return int(host(flag)[0])


def base_words(n, is_f32, seed=0):
    """Finite background: random finite values with the look-alike patterns sprinkled in."""
    rng = np.random.default_rng(seed + n)
    if is_f32:
        w = rng.standard_normal(n).astype(f32).view(np.uint32).copy()
        w[rng.integers(0, n, max(1, n // 5))] = rng.choice(np.array(FINITE32, np.uint32), max(1, n // 5))
    else:
        w = rng.standard_normal(n).astype(np.float16).view(np.uint16).copy()
        w[rng.integers(0, n, max(1, n // 5))] = rng.choice(np.array(FINITE16, np.uint16), max(1, n // 5))
    return w


@pytest.mark.parametrize("is_f32", [0, 1], ids=["f16", "f32"])
def test_found_inf_sees_every_position_of_the_tail_and_nothing_else(lib, is_f32):
    """n = 1 .. 9 (f16) / 1 .. 5 (f32) and sizes with whole 16-byte vectors in front: one non-finite value at every position is
    seen -- in either half of a 32-bit word, in the last vector, in the sub-16-byte tail -- and the finite look-alikes at every
    position (65504, FLT_MAX, 0x00007c00, 0x7c007c00, ... also in the float32 tail's even halfwords) are not."""
    per_vec = 4 if is_f32 else 8
    bad, fine = (BAD32, FINITE32) if is_f32 else (BAD16, FINITE16)
    sizes = list(range(1, per_vec + 2)) + [3 * per_vec + r for r in range(per_vec)]
    for n in sizes:
        w = base_words(n, is_f32)
        assert found_inf(lib, w, is_f32) == 0, n
        for pos in range(n):
            for k, value in enumerate(fine):
                x = w.copy(); x[pos] = value
                assert found_inf(lib, x, is_f32) == 0, (n, pos, hex(value))
            for k, value in enumerate(bad):
                x = w.copy(); x[pos] = value
                assert found_inf(lib, x, is_f32) == 1, (n, pos, hex(value))


@pytest.mark.parametrize("is_f32", [0, 1], ids=["f16", "f32"])
def test_found_inf_second_grid_stride_trip(lib, is_f32):
    """More than 2048 x 256 sixteen-byte vectors: first element, last element (in the tail), and one beyond the first trip."""
    per_vec = 4 if is_f32 else 8
    n = (2048 * 256 + 300) * per_vec + (per_vec - 1)
    w = base_words(n, is_f32)
    t = dev(w.view(np.int32 if is_f32 else np.int16))
    flag = flag_tensor(1)

    def check():
        lib.call("ngp_found_inf", lib.ptr(t), is_f32, n, lib.ptr(flag), 1, lib.stream())
        return int(host(flag)[0])
    assert check() == 0
    bad = (BAD32 if is_f32 else BAD16)
    for k, pos in enumerate((0, n - 1, 2048 * 256 * per_vec + 5 * per_vec + 1, n - per_vec)):
        keep = t[pos].clone()
        t[pos] = int(np.array([bad[k % len(bad)]], w.dtype).view(np.int32 if is_f32 else np.int16)[0])
        assert check() == 1, pos
        t[pos] = keep
    assert check() == 0


def test_found_inf_flag_behaviour(lib):
    fine, bad = base_words(37, 0), base_words(37, 0)
    bad[20] = 0x7C00
    assert found_inf(lib, fine, 0, flag_before=1, reset=0) == 1          # stays raised
    assert found_inf(lib, fine, 0, flag_before=1, reset=1) == 0          # cleared
    assert found_inf(lib, bad, 0, flag_before=0, reset=0) == 1
    assert found_inf(lib, bad, 0, flag_before=1, reset=1) == 1
    flag = flag_tensor(1)
    lib.call("ngp_found_inf", None, 0, 0, lib.ptr(flag), 1, lib.stream())   # n = 0 with reset: clears
    assert int(host(flag)[0]) == 0
    flag = flag_tensor(1)
    lib.call("ngp_found_inf", None, 0, 0, lib.ptr(flag), 0, lib.stream())
    assert int(host(flag)[0]) == 1


def found_inf2(lib, a, a_f32, b, b_f32, flag_before=0, clear_before=5):
    ta = dev(a.view(np.int32 if a_f32 else np.int16))
    tb = dev(b.view(np.int32 if b_f32 else np.int16)) if len(b) else None
    flag, clear = flag_tensor(flag_before), flag_tensor(clear_before)
    lib.call("ngp_found_inf2", lib.ptr(ta), a_f32, len(a), lib.ptr(tb), b_f32, len(b), lib.ptr(flag), lib.ptr(clear), lib.stream())
    return int(host(flag)[0]), int(host(clear)[0])


@pytest.mark.parametrize("a_f32,b_f32", [(0, 1), (1, 0), (0, 0), (1, 1)])
def test_found_inf2_boundary_types_and_flags(lib, a_f32, b_f32):
    """Two buffers of different types in one launch: a non-finite value on either side of the a / b boundary, at both ends and in
    either half of a word is seen by the test of ITS buffer's type; the look-alikes of the other type are not; flag_clear is
    written 0 and the flag is only ever raised."""
    na, nb = (4 if a_f32 else 8) * 3, (4 if b_f32 else 8) * 2
    a, b = base_words(na, a_f32, 1), base_words(nb, b_f32, 2)
    assert found_inf2(lib, a, a_f32, b, b_f32) == (0, 0)
    assert found_inf2(lib, a, a_f32, b, b_f32, flag_before=1) == (1, 0)              # never lowered
    assert found_inf2(lib, a, a_f32, b[:0], b_f32) == (0, 0)
    for buf, is_f32, which in ((a, a_f32, 0), (b, b_f32, 1)):
        for pos in (0, 1, len(buf) - 2, len(buf) - 1):
            for value in (BAD32 if is_f32 else BAD16):
                x = buf.copy(); x[pos] = value
                got = found_inf2(lib, x, a_f32, b, b_f32) if which == 0 else found_inf2(lib, a, a_f32, x, b_f32)
                assert got == (1, 0), (which, pos, hex(value))
            for value in (FINITE32 if is_f32 else FINITE16):
                x = buf.copy(); x[pos] = value
                got = found_inf2(lib, x, a_f32, b, b_f32) if which == 0 else found_inf2(lib, a, a_f32, x, b_f32)
                assert got == (0, 0), (which, pos, hex(value))
    flag, ta = flag_tensor(0), dev(a.view(np.int32 if a_f32 else np.int16))
    lib.call("ngp_found_inf2", lib.ptr(ta), a_f32, na, None, b_f32, 0, lib.ptr(flag), None, lib.stream())
    assert int(host(flag)[0]) == 0                                                   # flag_clear = NULL is allowed


def test_found_inf2_second_grid_stride_trip(lib):
    """a (f16) fills the first trip of 2048 x 256 vectors; b (f32) lies wholly beyond it."""
    na, nb = 2048 * 256 * 8 + 64, 4 * 50
    a, b = base_words(na, 0, 4), base_words(nb, 1, 5)
    ta, tb = dev(a.view(np.int16)), dev(b.view(np.int32))

    def check():
        flag, clear = flag_tensor(0), flag_tensor(9)
        lib.call("ngp_found_inf2", lib.ptr(ta), 0, na, lib.ptr(tb), 1, nb, lib.ptr(flag), lib.ptr(clear), lib.stream())
        return int(host(flag)[0]), int(host(clear)[0])
    assert check() == (0, 0)
    tb[nb - 1] = int(np.array([0xFF800000], np.uint32).view(np.int32)[0])
    assert check() == (1, 0)
    tb[nb - 1] = 0
    ta[na - 3] = int(np.array([0xFC00], np.uint16).view(np.int16)[0])
    assert check() == (1, 0)
    ta[na - 3] = 0
    assert check() == (0, 0)
