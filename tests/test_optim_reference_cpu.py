"""Proves tests/optim_reference.py on the CPU: the float64 restatements are the operations they claim to be (against torch in
float64), and the derived bounds hold for an uncontracted float32 evaluation of the same expressions on every case that
tests/test_optim_exact_gpu.py runs -- so a failure there is the kernel's, not the reference's."""
import numpy as np
import pytest
import torch

from tests import optim_reference as R

f32, f64 = np.float32, np.float64


def test_adam_ref_is_adamw_in_float64():
    """Five steps of adam_ref (values only) == torch.optim.AdamW in float64, rtol 1e-12, with weight decay (the same decoupled
    rule).  AdamW is handed the float32 coefficients as doubles; it forms its bias corrections 1 - beta^t in double, so the
    reference runs with those instead of its float32 ones here (test_float32_bias_corrections_against_apex has the difference)."""
    rng = np.random.default_rng(3)
    n = 4096
    p = rng.standard_normal(n).astype(f32); m = np.zeros(n, f32); v = np.zeros(n, f32)
    ref = torch.tensor(p.astype(f64), requires_grad=True)
    c0 = R.AdamCoef(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-15, wd=1e-2, step=1, grad_scale=1.0)
    opt = torch.optim.AdamW([ref], lr=c0.lr, betas=(c0.beta1, c0.beta2), eps=c0.eps, weight_decay=c0.wd)
    p64, m64, v64 = p.astype(f64), m.astype(f64), v.astype(f64)
    for t in range(1, 6):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(f32)
        c = R.AdamCoef(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-15, wd=1e-2, step=t, grad_scale=1.0)
        c.bc1, c.bc2 = 1.0 - c.beta1 ** t, 1.0 - c.beta2 ** t               # AdamW's own (double) corrections
        (p64, m64, v64), _ = R.adam_ref(p64, m64, v64, g, c)
        ref.grad = torch.tensor(g.astype(f64))
        opt.step()
        # AdamW divides sqrt(v) by sqrt(bc2) and adds eps; the kernel takes sqrt(v / bc2) + eps: the same number in exact arithmetic
        np.testing.assert_allclose(p64, ref.detach().numpy(), rtol=1e-12, atol=0)
    st = opt.state[ref]
    np.testing.assert_allclose(m64, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(v64, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)


def test_grad_scale_and_weight_decay_sit_where_the_rule_puts_them():
    """The pieces the AdamW comparison cannot see: g = g_raw / grad_scale, and the decay term is lr wd p (decoupled: not in m, v)."""
    rng = np.random.default_rng(4)
    p, m, v = rng.standard_normal(64), rng.standard_normal(64) * 1e-2, rng.random(64) * 1e-3
    g = rng.standard_normal(64)
    a = R.adam_ref(p, m, v, g * 128.0, R.AdamCoef(wd=0.0, step=3, grad_scale=128.0))[0]
    b = R.adam_ref(p, m, v, g, R.AdamCoef(wd=0.0, step=3, grad_scale=1.0))[0]
    for x, y in zip(a, b):
        np.testing.assert_allclose(x, y, rtol=1e-15)
    c = R.AdamCoef(wd=1e-2, step=3)
    w = R.adam_ref(p, m, v, g, c)[0]
    np.testing.assert_allclose(w[0], b[0] - c.lr * c.wd * p, rtol=1e-14)
    assert np.array_equal(w[1], b[1]) and np.array_equal(w[2], b[2])


@pytest.mark.parametrize("grad_is_f32", [False, True])
def test_uncontracted_float32_adam_stays_inside_the_bound(grad_is_f32):
    """Every dense case of the GPU test (all sizes, steps, weight decays, grad scales, the specials) evaluated in numpy float32:
    inside the bound for every element, so the reference alone satisfies the condition it sets."""
    worst = np.zeros(3)
    for n in R.ADAM_SIZES + (65536 + 7,):           # (the large GPU size has the same element recipe; a slice of it is enough here)
        for t, wd, gs in R.adam_combos():
            p, m, v, g, kind = R.adam_dense_inputs(n, grad_is_f32, gs)
            c = R.AdamCoef(wd=wd, step=t, grad_scale=gs)
            if grad_is_f32:
                got = R.adam_f32(p, m, v, g, c)
            else:
                gc, nan = R.clamp_f16_grad(g)
                got = R.adam_f32(p, m, v, np.where(nan, -R.F16_MAX, gc).astype(f32), c)     # fmaxf(NaN, -65504) = -65504
            assert all(np.isfinite(x).all() for x in got)
            fr = R.worst_fraction(got, R.adam_dense_reference(p, m, v, g, c))
            assert max(fr) <= 1.0, (n, t, wd, gs, fr)
            worst = np.maximum(worst, fr)
            zero = kind == 0
            if wd == 0.0 and zero.any():
                assert np.array_equal(got[0][zero].view(np.uint32), p[zero].view(np.uint32))
    print("worst fraction of (e_p, e_m, e_v) reached by uncontracted float32:", worst)
    assert worst.min() > 0.05, worst             # the bound is not vacuous: float32 comes within a factor 20 of it


def test_uncontracted_float32_partials_adam_stays_inside_the_bound():
    worst = np.zeros(3)
    for n_partials in R.PARTIALS_ROWS:
        for n in R.PARTIALS_N:
            t, wd, gs = R.partials_combo(n_partials, n)
            p, m, v, rows = R.partials_inputs(n_partials, n)
            c = R.AdamCoef(wd=wd, step=t, grad_scale=gs)
            got = R.adam_partials_f32(p, m, v, rows, c)
            fr = R.worst_fraction(got, [R.adam_partials_reference(p, m, v, rows, c)])
            assert max(fr) <= 1.0, (n_partials, n, fr)
            worst = np.maximum(worst, fr)
    print("partials: worst fraction of (e_p, e_m, e_v):", worst)


def test_a_dropped_or_repeated_row_breaks_the_partials_bound():
    """The rows are built so that the summation bound is orders of magnitude below one row's contribution."""
    for n_partials in (9, 17, 33):
        p, m, v, rows = R.partials_inputs(n_partials, 33)
        c = R.AdamCoef(wd=1e-2, step=2, grad_scale=128.0)
        alts = [R.adam_partials_reference(p, m, v, rows, c)]
        for bad in (rows[:-1], np.concatenate([rows, rows[-1:]])):
            fr = R.worst_fraction(R.adam_partials_f32(p, m, v, bad, c), alts)
            assert min(fr) > 100.0, fr


def test_float32_bias_corrections_against_apex():
    """t = 1 .. 35000: fl32(1 - fl32(beta^t)) against apex's 1 - beta**t in double (beta the float32 the launcher receives),
    rounded to float32.  Where beta^t >= 1/2 the float32 subtraction is exact and the two differ by at most ulp32(beta^t) / bc;
    below 1/2 each side is rounded at bc's spacing, which is then the larger one: ulp32(beta^t) + ulp32(bc).  Largest relative
    deviation: 1.1e-7 of bc1 (t = 11 .. 31) and 6.7e-6 of bc2 (t around 450, bc2 = 0.36 -- where 1 - beta2^t has lost four bits to
    cancellation); the update moves by that much of itself through bc1 and by half of it through bc2.  A documented deviation
    from apex, not a tolerance of the GPU test: there the reference takes the float32 corrections themselves."""
    steps = np.arange(1, 35001)
    for beta, largest in ((0.9, 1.2e-7), (0.999, 7e-6)):
        diff, ulp_pw, ulp_bc, bc = R.bias_correction_deviation(beta, steps)
        hi = ulp_pw >= 2.0 ** -24                      # beta^t >= 1/2
        assert hi.any() and not hi.all()
        assert np.all(diff[hi] <= ulp_pw[hi])
        assert np.all(diff[~hi] <= ulp_pw[~hi] + ulp_bc[~hi])
        assert (diff / bc).max() <= largest, (diff / bc).max()


def test_merge_gradient_saturates_and_sums_in_part_order():
    partial = np.zeros((8 + 2 * 2, 2), f32)
    partial[0] = (70000.0, -1e9)                       # level 0, one part: saturates
    partial[8] = (60000.0, 1.0); partial[10] = (6000.0, 2.0 ** -12)        # level 1 entry 0: two parts
    got = R.merge_gradient(partial, [0, 8, 10], [1, 2], [0, 8])
    assert got.dtype == np.float16 and got.shape == (20,)
    assert got[0] == 65504.0 and got[1] == -65504.0 and got[16] == 65504.0 and got[17] == 1.0


def _loss_inputs(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3)), rng.choice(R.log_sweep(), n).astype(f64), rng.random((n, 3)), np.array([0.2, 0.7, 1.0])


@pytest.mark.parametrize("with_bg", [True, False])
def test_loss_seeds_are_the_float64_autograd_of_the_loss(with_bg):
    """nerf_loss_ref == ngp_pl_amd.losses.mean_loss_and_seeds in float64, and its seeds == torch autograd of its loss, to 1e-12."""
    from ngp_pl_amd.losses import mean_loss_and_seeds
    n = 777
    rgb, o, gt, bg = _loss_inputs(n)
    bg = bg if with_bg else None
    ref = R.nerf_loss_ref(rgb, o, gt, bg, 1e-3, 128.0)
    lam = float(f32(1e-3))
    # the reference forms o + 1e-10 in float32 first; hand torch the same opacities shifted so that its o + 1e-10 is that value
    oe = (o.astype(f32) + R.LOSS_EPS).astype(f64)
    t_rgb = torch.tensor(rgb, requires_grad=True)
    t_oe = torch.tensor(oe, requires_grad=True)
    tbg = None if bg is None else torch.tensor(bg)
    blended = t_rgb if bg is None else t_rgb + tbg.view(1, 3) * (1.0 - torch.tensor(o)).unsqueeze(1)
    loss = ((blended - torch.tensor(gt)) ** 2).sum() / (3 * n) + (-lam * t_oe * torch.log(t_oe)).sum() / n
    g_rgb, g_oe = torch.autograd.grad(loss, [t_rgb, t_oe])
    np.testing.assert_allclose(ref["loss"], float(loss.detach()), rtol=1e-12)
    np.testing.assert_allclose(ref["d_rgb"], 128.0 * g_rgb.numpy(), rtol=1e-12, atol=1e-300)
    d_o = g_oe.numpy()
    if bg is not None:                                  # the blend's own dependence on the opacity
        d_o = d_o - (g_rgb.numpy() * bg[None, :]).sum(1)
    np.testing.assert_allclose(ref["d_o"], 128.0 * d_o, rtol=1e-12, atol=1e-18)
    # ... and the package's own torch statement, in float64 (its o + 1e-10 is formed in float64: equal to ~1e-7 relative in the log)
    mine = mean_loss_and_seeds(torch.tensor(rgb), torch.tensor(o), torch.tensor(gt), tbg, lam, 128.0)
    np.testing.assert_allclose(ref["sq_err"], float(mine[1]), rtol=1e-12)
    np.testing.assert_allclose(ref["d_rgb"], mine[2].numpy(), rtol=1e-12, atol=1e-300)
    keep = o > 1e-3                                     # (where 1e-10 against o is below the float32 rounding of the sum)
    np.testing.assert_allclose(ref["d_o"][keep], mine[3].numpy()[keep], rtol=1e-5, atol=1e-12)


def _nerf_loss_f32(rgb, o, gt, bg, lam, gs):
    """nerf_loss_ray in uncontracted numpy float32 (the logarithm: float64, rounded)."""
    rgb, o, gt = rgb.astype(f32), o.astype(f32), gt.astype(f32)
    n = o.shape[0]
    lam, gs = f32(lam), f32(gs)
    inv_r, inv_3r = f32(1) / f32(n), f32(1) / (f32(3) * f32(n))
    go = np.zeros(n, f32); se = np.zeros(n, f32); d_rgb = np.zeros((n, 3), f32)
    for k in range(3):
        b = f32(0 if bg is None else bg[k])
        diff = rgb[:, k] + b * (f32(1) - o) - gt[:, k]
        se = se + diff * diff
        gr = f32(2) * diff * inv_3r
        d_rgb[:, k] = gr * gs
        go = go - gr * b
    oe = o + R.LOSS_EPS
    lg = np.log(oe.astype(f64)).astype(f32)
    l = se * inv_3r + lam * (-oe * lg) * inv_r
    go = go + lam * (-(lg + f32(1))) * inv_r
    return l, se, d_rgb, go * gs


@pytest.mark.parametrize("with_bg", [True, False])
@pytest.mark.parametrize("n", [1, 257, 16385])
def test_uncontracted_float32_loss_stays_inside_the_bounds(n, with_bg):
    rgb, o, gt, bg = _loss_inputs(n, 1)
    bg = bg if with_bg else None
    ref = R.nerf_loss_ref(rgb.astype(f32), o, gt.astype(f32), None if bg is None else bg.astype(f32), 1e-3, 128.0, tau=1.0)
    l, se, d_rgb, d_o = _nerf_loss_f32(rgb, o, gt, bg, 1e-3, 128.0)
    assert np.all(np.abs(d_rgb - ref["d_rgb"]) <= ref["e_d_rgb"])
    assert np.all(np.abs(d_o - ref["d_o"]) <= ref["e_d_o"])
    k = R.loss_reduction_k(n)
    assert abs(float(l.astype(f64).sum()) - ref["loss"]) <= ref["e_l"]                      # (per-ray errors alone: summed in float64)
    assert abs(float(np.sum(l, dtype=f32)) - ref["loss"]) <= ref["e_l"] + k * R.E * np.abs(ref["l_ray"]).sum() or n > 16384
    assert abs(float(se.astype(f64).sum()) - ref["sq_err"]) <= ref["e_se"]


def test_overwrite_sum_tree_tells_workgroup_order_from_arrival_order():
    """The pattern of the GPU test's order check: one workgroup's partial is large, the others' are 0.3 of its ulp.  The tree of
    nerf_loss_kernel<OVERWRITE> collects them in groups (19 ulp in all); adding them one by one to the large one loses them all."""
    per_ray = np.zeros(16384, f32)
    per_ray[0] = 1.0
    per_ray[256::256] = f32(0.3 * 2.0 ** -23)
    total, parts = R.overwrite_sum_f32(per_ray)
    assert parts[0] == 1.0 and np.all(parts[1:] == f32(0.3 * 2.0 ** -23))
    serial = f32(1.0)
    for x in parts[1:]:
        serial = serial + x
    assert serial == 1.0 and total > 1.0 + 15 * 2.0 ** -23


def test_terms_and_blend_references():
    rgb, o, gt, bg = _loss_inputs(300, 2)
    fw = R.loss_terms_ref(rgb, o, gt, 1.0)
    bw = R.loss_terms_bw_ref(0.5, 2.0, rgb, o, gt, 1.0)
    oe = torch.tensor((o.astype(f32) + R.LOSS_EPS).astype(f64), requires_grad=True)
    t_rgb = torch.tensor(rgb, requires_grad=True)
    sq = (t_rgb - torch.tensor(gt)) ** 2
    ent = -oe * torch.log(oe)
    np.testing.assert_allclose(fw["sq"], sq.detach().numpy(), rtol=1e-13)
    np.testing.assert_allclose(fw["ent"], ent.detach().numpy(), rtol=1e-12, atol=1e-300)
    g_rgb, g_o = torch.autograd.grad(0.5 * sq.sum() + 2.0 * ent.sum(), [t_rgb, oe])
    np.testing.assert_allclose(bw["g_rgb"], g_rgb.numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(bw["g_opacity"], g_o.numpy(), rtol=1e-12, atol=1e-15)
    out = R.bg_blend_ref(rgb.astype(f32), o.astype(f32), bg.astype(f32))
    np.testing.assert_allclose(out, rgb.astype(f32) + bg.astype(f32)[None] * (1 - o.astype(f32))[:, None], rtol=1e-6)
    g, e = R.bg_blend_bw_ref(rgb, o, bg)
    np.testing.assert_allclose(g, o - rgb @ bg, rtol=1e-12, atol=1e-15)
    g0, _ = R.bg_blend_bw_ref(rgb, None, bg)
    np.testing.assert_allclose(g0, -(rgb @ bg), rtol=1e-12)


def test_cast_inputs_cover_what_they_name():
    x = R.cast_inputs()
    assert 330_000 <= x.shape[0] <= 400_000 and x.dtype == f32
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    assert np.isinf(h[x == f32(65520.0)]).all() and (h[x == f32(65519.996)] == 65504.0).all()          # the last tie rounds to inf
    assert (h[x == f32(2.0 ** -25)] == 0).all() and (h[x == np.nextafter(f32(2.0 ** -25), f32(1))] == 2.0 ** -24).any()
    fin = np.isfinite(x) & np.isfinite(h)
    assert np.count_nonzero(x[fin] != h[fin].astype(f32)) > 200_000                                    # most inputs are inexact


def test_sum_slices_ref_rounds_once_and_ignores_the_poisoned_slice():
    own = np.array([2048.0, 40000.0, 1.0, 0.0] * 2, np.float16)
    stage = np.zeros((2, 8), np.float16)
    stage[0] = np.nan                                   # rank 0's own slot in stage: ignored
    stage[1] = np.array([1.0, 40000.0, 2050.0, 0.0] * 2, np.float16)
    got = R.sum_slices_ref(own, stage, 0)
    assert got[0] == 2048.0 and np.isinf(got[1]) and got[2] == 2052.0 and got[3] == 0.0     # ties to even, no saturation


def test_reduce_bound_holds_for_the_kernel_order():
    for n_partials in R.REDUCE_ROWS:
        rows = R.partials_inputs(n_partials, 33)[3]
        lanes = np.zeros((8, 33), f32)
        for r in range(8):
            acc = [np.zeros(33, f32) for _ in range(4)]
            q = r
            while q + 24 < n_partials:
                for j in range(4):
                    acc[j] = acc[j] + rows[q + 8 * j]
                q += 32
            while q < n_partials:
                acc[0] = acc[0] + rows[q]
                q += 8
            lanes[r] = (acc[0] + acc[1]) + (acc[2] + acc[3])
        t = np.zeros(33, f32)
        for r in range(8):
            t = t + lanes[r]
        want = rows.astype(f64).sum(0) if n_partials else np.zeros(33)
        assert np.all(np.abs(t - want) <= R.reduce_bound(rows.astype(f64).reshape(n_partials, 33), 10))
