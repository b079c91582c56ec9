"""No GPU: the reference of tests/field_forward_reference.py is shown to be sound, to refuse wrong kernels and not to be vacuous, on the
cases of tests/field_forward_cases.py that tests/test_field_forward_exact_gpu.py runs on the device.

  * its midpoint agrees with oracle/tcnn_oracle.py evaluated in float64 with the f16 rounding points (quantize=True);
  * the emulation of the kernel (a k-ordered f32 chain per layer) lies inside every interval in three K orders, on every case;
  * the exact nets satisfy their exactness condition and all three orders give the expected bits on them, as on the one-hot cases;
  * nine wrong kernels, restated as mutations of the emulation, are refused by the SAME check function the GPU test calls, each on a
    large share of the outputs it touches (floors below, next to what was measured);
  * the intervals are narrow: per network the share that is a single f16 value, and at most 1 and at most 4 f16 spacings wide, is
    printed and held to floors 10 % (relative) below what the reference gives on the committed cases.  These floors are conditions on
    the INPUTS (how much room an unknown summation order gets), not measurements of the kernel."""
import numpy as np
import pytest
import torch

from oracle import tcnn_oracle as T
from tests import field_forward_cases as K
from tests import field_forward_reference as F

N = 8000
ROWS = np.arange(N)


def ws_of(n_in, n_hidden, kind):
    return F.split_weights(K.weights(n_in, n_hidden, kind), n_in, n_hidden)


def field_ws(kind):
    dw, rw = K.field_weights(kind)
    return F.split_weights(dw, 32, 1), F.split_weights(rw, 32, 2)


def field_emulation(kind, order, mut=None, rows=ROWS, src=None):
    dws, rws = field_ws(kind)
    src = rows if src is None else src                       # src != rows: outputs of `rows` computed from the inputs of `src`
    return F.emulate_field(dws, rws, K.field_feats()[src], K.field_dirs()[src], order, mut)


# ---------------------------------------------------------------------------------------------------------------- the reference is sound
@pytest.mark.parametrize("n_in,n_hidden", K.CONFIGS)
def test_midpoint_agrees_with_the_oracle(n_in, n_hidden):
    for kind in K.WEIGHT_KINDS:
        blob, x = K.weights(n_in, n_hidden, kind), K.inputs(n_in)[:N]
        ref = K.mlp_reference(n_in, n_hidden, kind)
        for act, lo, hi in ((0, ref.lo, ref.hi), (1, ref.act_lo, ref.act_hi)):
            want = T.mlp(torch.from_numpy(x.astype(np.float64)), torch.from_numpy(blob.astype(np.float64)), n_in, n_hidden, 16,
                         "Sigmoid" if act else "None", quantize=True, dtype=torch.float64)
            assert want.dtype == torch.float64
            res = F.check(F.f16(want.numpy()), lo[:N], hi[:N], "oracle %d-%d %s act %d" % (n_in, n_hidden, kind, act))
            assert res.bad == 0, res.worst
            mid = F.forward_point(ws_of(n_in, n_hidden, kind), x)
            if act == 0:
                assert F.check(mid, lo[:N], hi[:N]).bad == 0
                # the two float64 evaluations agree but where a hidden sum sits next to an f16 midpoint (torch rounds float64 to f16
                # through f32) and flips by one spacing
                assert (F.ord16(mid) == F.ord16(F.f16(want.numpy()))).mean() > 0.99


@pytest.mark.parametrize("kind", K.FIELD_KINDS)
def test_field_midpoint_agrees_with_the_oracle(kind):
    dw, rw = K.field_weights(kind)
    feats, d = K.field_feats()[:N], K.field_dirs()[:N]
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    h = T.q16(T.mlp(t(feats), t(dw), 32, 1, 16, "None", quantize=True, dtype=torch.float64))
    dn = t(d) / torch.norm(t(d), dim=1, keepdim=True)
    sh = T.q16(T.sh4(dn))
    rgb = T.mlp(torch.cat([sh, h], 1), t(rw), 32, 2, 3, "Sigmoid", quantize=True, dtype=torch.float64)
    h16 = F.f16(h.numpy())
    sigma = np.exp(h16[:, 0].astype(np.float64)).astype(np.float32)
    rgb16 = F.f16(rgb.numpy()).astype(np.float32)
    for res in K.check_field(kind, ROWS, h16, sigma, rgb16, "oracle field " + kind):
        assert res.bad == 0, res.worst
    sh_lo, sh_hi = F.sh_interval(d)
    assert F.check(F.f16(T.sh4(dn).numpy()), sh_lo, sh_hi, "oracle SH").bad == 0


@pytest.mark.parametrize("order", F.ORDERS)
@pytest.mark.parametrize("n_in,n_hidden", K.CONFIGS)
def test_emulated_mlp_is_inside_every_interval(n_in, n_hidden, order):
    for kind in K.WEIGHT_KINDS:
        ref = K.mlp_reference(n_in, n_hidden, kind)
        for rows in (ROWS, np.arange(K.N_MAX - 300, K.N_MAX)):
            x = K.inputs(n_in)[rows]
            for act, lo, hi in ((0, ref.lo, ref.hi), (1, ref.act_lo, ref.act_hi)):
                got = F.emulate_mlp(ws_of(n_in, n_hidden, kind), x, order, act)
                res = F.check(got, lo[rows], hi[rows], "emulated %d-%d %s %s act %d" % (n_in, n_hidden, kind, order, act))
                assert res.bad == 0, res.worst


@pytest.mark.parametrize("order", F.ORDERS)
@pytest.mark.parametrize("kind", K.FIELD_KINDS)
def test_emulated_field_is_inside_every_interval(kind, order):
    for rows in (ROWS, np.arange(K.N_MAX - 300, K.N_MAX)):
        h, sigma, rgb = field_emulation(kind, order, rows=rows)
        for res in K.check_field(kind, rows, h, sigma, rgb, "emulated field %s %s" % (kind, order)):
            assert res.bad == 0, res.worst
        # without h: sigma against the h interval
        ref = K.density_reference(kind)
        res = F.check_sigma(sigma, ref.lo[rows, 0], ref.hi[rows, 0])
        assert res.bad == 0, res.worst


@pytest.mark.parametrize("order", F.ORDERS)
def test_emulated_sigma_edges(order):
    c = K.sigma_edge_case()
    h, sigma, rgb = F.emulate_field(F.split_weights(c.density_w, 32, 1), F.split_weights(c.rgb_w, 32, 2), c.feats, c.dirs, order)
    rows = np.arange(c.n)
    for res in K.check_field("trained", rows, h, sigma, rgb, "emulated sigma edges", dirs=c.dirs, ref=c.ref, rgb_w=c.rgb_w):
        assert res.bad == 0, res.worst
    h0 = h[:, 0].astype(np.float64)
    assert np.array_equal(h0, c.feats[:, 0].astype(np.float64))
    assert np.isposinf(sigma[h0 >= 89]).all() and (h0 >= 89).sum() > 100
    assert (sigma[h0 <= -104] == 0).all() and (h0 <= -104).sum() > 100
    assert ((h0 > -104) & (h0 < -87.34)).sum() > 100 and np.isfinite(sigma[h0 <= 88.6875]).all()


def test_sigma_range_rules():
    lo, hi, flush = F.sigma_interval(np.array([89.0, 88.6875, -104.0, -103.9375, -90.0, -87.0, 11.0]))
    assert np.isposinf(lo[0]) and np.isposinf(hi[0]) and np.isfinite(lo[1]) and hi[1] < F.F32_MAX
    assert lo[2] == 0 and hi[2] == 0 and hi[3] > 0 and list(flush[2:]) == [True, True, True, False, False]
    # a flushed zero passes only where the value is subnormal; a NaN, a wrong sign and a non-zero below -104 never do
    assert F.check_sigma(np.array([0, 0, 0, 0], np.float32), np.array([-90.0, -87.0, -104.0, 11.0])).bad == 2
    assert F.check_sigma(np.array([np.nan, -1e-40, 1e-45, np.inf], np.float32), np.array([-90.0, -90.0, -104.0, 88.0])).bad == 4
    assert F.check_sigma(np.array([np.exp(11.0) * (1 + 2e-6), np.exp(11.0) * (1 - 2e-6)]), np.array([11.0, 11.0])).bad == 2
    assert F.check_sigma(np.array([np.exp(11.0)], np.float32), np.array([11.0])).bad == 0


def test_sh_interval():
    d = K.field_dirs()[:N]
    lo, hi = F.sh_interval(d)
    res = F.check(F.sh4_f32(d), lo, hi, "f32 SH")
    print("\nSH input chunk: %.2f %% single-valued intervals, %.2f %% at most 1 wide" % (100 * res.single, 100 * res.le1))
    assert res.bad == 0, res.worst
    assert res.single >= 0.9
    # the poles and the axes: exact zeros stay exact, whatever the norm
    val, mass = F.sh_exact(np.array([[0, 0, 1e3], [0, 0, -1e-3], [2, 0, 0]], np.float32))
    assert (val[0, [1, 3, 4, 5, 7, 8, 9, 10, 11, 13, 14, 15]] == 0).all() and (mass[0, [1, 3, 4, 5, 7]] == 0).all()
    assert abs(val[0, 6] - 0.6307831305) < 1e-7 and abs(val[1, 2] + 0.4886025119) < 1e-7 and abs(val[2, 3] + 0.4886025119) < 1e-7
    with pytest.raises(ValueError):
        F.sh_exact(np.zeros((1, 3), np.float32))


# ---------------------------------------------------------------------------------------------------------------- exact nets, one-hot inputs
@pytest.mark.parametrize("n_in,n_hidden", K.CONFIGS)
def test_exact_nets(n_in, n_hidden):
    blob, x, want = F.exact_net(n_in, n_hidden, 300, seed=n_in + n_hidden)
    ws = F.split_weights(blob, n_in, n_hidden)
    assert F.exactness_holds(ws, x)
    assert not F.exactness_holds(ws_of(n_in, n_hidden, "trained"), K.inputs(n_in)[:50])
    assert np.abs(want.astype(np.float64)).max() > 8 and (want != 0).mean() > 0.5          # dense, and not small
    assert np.array_equal(F.forward_point(ws, x).view(np.int16), want.view(np.int16))
    ref = F.mlp_intervals(ws, x)
    assert F.check(want, ref.lo, ref.hi).bad == 0
    for order in F.ORDERS:
        got = F.emulate_mlp(ws, x, order)
        assert np.array_equal(got.view(np.int16), want.view(np.int16)), order
    # the condition matters: the same net with inputs 64 times larger breaks it, and the condition says so
    assert not F.exactness_holds(ws, (x.astype(np.float64) * 64 + 2.0 ** -3).astype(np.float16))


@pytest.mark.parametrize("n_in,n_hidden", K.CONFIGS)
def test_one_hot_cases(n_in, n_hidden):
    covered = 0
    for name, blob, x, want in K.one_hot_cases(n_in, n_hidden):
        ws = F.split_weights(blob, n_in, n_hidden)
        ref = F.mlp_intervals(ws, x)
        assert F.check(want, ref.lo, ref.hi, name).bad == 0
        for order in F.ORDERS:
            got = F.emulate_mlp(ws, x, order)
            assert np.array_equal(got.view(np.int16), want.view(np.int16)), (name, order)
        covered += int((want != 0).sum())
    assert covered > 1000


# ---------------------------------------------------------------------------------------------------------------- wrong kernels are refused
# Floors: the share of outputs outside their interval that a mutant must reach at least.  Next to each, what was measured on the
# committed cases (N = 8000 rows, trained-like weights, the kernel's K order).
MLP_FLOORS = {            # measured over the six networks, 16-64-16 ... 64-64-64-16
    "truncate": 0.10,         # f32 -> f16 toward zero:                          75.9 67.5 70.9 49.8 56.6 19.3 %
    "drop_first": 0.50,       # one product of the first layer left out:         99.5 99.1 99.1 97.9 98.5 96.0 %
    "drop_out": 0.20,         # one product of the output layer left out:        49.6 57.5 50.2 89.4 49.0 34.0 % (the unit is 0 for half)
    "chunk_natural": 0.50,    # one K chunk's weights in natural order, not D:   99.2 99.5 99.6 99.2 99.5 99.1 %
}


@pytest.mark.parametrize("mut", sorted(MLP_FLOORS))
@pytest.mark.parametrize("n_in,n_hidden", K.CONFIGS)
def test_wrong_mlp_kernels_are_refused(n_in, n_hidden, mut):
    ref = K.mlp_reference(n_in, n_hidden, "trained")
    ws, x = ws_of(n_in, n_hidden, "trained"), K.inputs(n_in)[:N]
    honest = F.check(F.emulate_mlp(ws, x, "kernel"), ref.lo[:N], ref.hi[:N])
    assert honest.bad == 0
    res = F.check(F.emulate_mlp(ws, x, "kernel", 0, mut), ref.lo[:N], ref.hi[:N], "%s %d-%d" % (mut, n_in, n_hidden))
    print("\n%-16s %d-%d: %.1f %% of outputs outside their interval" % (mut, n_in, n_hidden, 100 * res.share_bad))
    assert res.share_bad >= MLP_FLOORS[mut], res.worst


FIELD_FLOORS = {          # mutant: (which result: 0 h, 1 sigma, 2 rgb; floor)      measured outside: h / sigma / rgb
    "truncate": (0, 0.10),            # 69.4 /  0.0 / 26.2 %
    "drop_first": (0, 0.50),          # 99.4 /  0.0 / 97.1 %
    "drop_out": (0, 0.20),            # 50.5 /  0.0 / 36.0 %
    "chunk_natural": (2, 0.50),       # 99.7 /  0.0 / 99.5 %   (rgb: the colour net's second layer, from the mutant's own h)
    "sigma_unrounded": (1, 0.50),     #  0.0 / 98.9 /  0.0 %   sigma = exp(f32 accumulator), not exp(f16 h[0])
    "rgb_unrounded": (2, 0.50),       #  0.0 /  0.0 / 100  %   rgb not rounded to f16: no f16 value
    "sh_unnormalised": (2, 0.50),     #  0.0 /  0.0 / 99.7 %   SH of d, not of d / |d|
}


@pytest.mark.parametrize("mut", sorted(FIELD_FLOORS))
def test_wrong_field_kernels_are_refused(mut):
    which, floor = FIELD_FLOORS[mut]
    h, sigma, rgb = field_emulation("trained", "kernel", mut)
    res = K.check_field("trained", ROWS, h, sigma, rgb, mut)
    print("\n%-16s field: outside their interval: h %.1f %%, sigma %.1f %%, rgb %.1f %%" % (mut, 100 * res[0].share_bad, 100 * res[1].share_bad, 100 * res[2].share_bad))
    assert res[which].share_bad >= floor, res[which].worst


def test_an_unwritten_last_tile_is_refused():
    """The kernel leaves the last (partial) tile of a launch of 65 536 + 129 samples unwritten: the prefill, a NaN, stays there.  EVERY
    output of that tile must count as outside (the share is of the tile: one tile is all this mutant touches)."""
    n = 65536 + 129
    rows = np.arange(n - 300, n)
    h, sigma, rgb = field_emulation("trained", "kernel", rows=rows)
    tile = rows >= (n - 1) // F.TILE * F.TILE
    assert tile.sum() == 1
    h[tile], sigma[tile], rgb[tile] = np.float16(np.nan), np.float32(np.nan), np.float32(np.nan)
    res = K.check_field("trained", rows, h, sigma, rgb, "unwritten tile")
    assert res[0].bad == 16 * tile.sum() and res[1].bad == tile.sum() and res[2].bad == 3 * tile.sum()
    n = 65536 + 31                                                                     # the same with a fuller tile
    rows = np.arange(n - 300, n)
    out = F.emulate_mlp(ws_of(32, 2, "trained"), K.inputs(32)[rows], "kernel")
    tile = rows >= (n - 1) // F.TILE * F.TILE
    assert tile.sum() == 31
    out[tile] = np.float16(np.nan)
    ref = K.mlp_reference(32, 2, "trained")
    assert F.check(out, ref.lo[rows], ref.hi[rows]).bad == 16 * 31


def test_a_second_sweep_from_the_first_sweeps_inputs_is_refused():
    """Tiles of the second sweep (samples 65 536 ...) computed from the inputs of the tile one sweep earlier, as a prefetch that is not
    advanced would: measured 100 % of the second sweep's h and 99.7 % of its rgb outside; floor 0.5."""
    rows = np.arange(F.SWEEP, F.SWEEP + 129)
    h, sigma, rgb = field_emulation("trained", "kernel", rows=rows, src=rows - F.SWEEP)
    ref = K.density_reference("trained")
    res = F.check(h, ref.lo[rows], ref.hi[rows], "stale inputs")
    print("\nstale inputs: %.1f %% of the second sweep's h outside" % (100 * res.share_bad))
    assert res.share_bad >= 0.5
    # rgb is held against the launch's own h: what gives a stale tile away there are the directions
    _, _, rr = K.check_field("trained", rows, h, sigma, rgb, "stale inputs")
    print("stale inputs: %.1f %% of the second sweep's rgb outside" % (100 * rr.share_bad))
    assert rr.share_bad >= 0.5
    x = K.inputs(64)
    out = F.emulate_mlp(ws_of(64, 1, "trained"), x[rows - F.SWEEP], "kernel")
    mref = K.mlp_reference(64, 1, "trained")
    assert F.check(out, mref.lo[rows], mref.hi[rows]).share_bad >= 0.5


def test_the_check_counts_every_output():
    lo, hi = np.array([1.0, 1.0, 1.0, -0.0], np.float16), np.array([1.0, 1.001, 2.0, 0.0], np.float16)
    res = F.check(np.array([1.0, 1.0, 1.5, 0.0], np.float16), lo, hi)
    assert res.bad == 0 and res.n == 4 and res.single == 0.5 and res.le1 == 0.75
    for v in (np.nan, np.inf, 2.002, 0.999):
        assert F.check(np.array([1.0, 1.0, v, 0.0], np.float16), lo, hi).bad == 1
    r = F.check_rgb(np.array([[0.5, 0.50001, 0.25]], np.float32), np.array([[0.5, 0.5, 0.25]], np.float16), np.array([[0.5, 0.501, 0.25]], np.float16))
    assert r.bad == 1 and r.not_f16 == 1


# ---------------------------------------------------------------------------------------------------------------- the intervals are narrow
# (single, <= 1, <= 4) measured on all N_MAX rows of the committed case; the floors are 10 % (relative) below.
MEASURED_WIDTHS = {
    "16-64-16 trained": (0.6555, 0.9133, 0.9719), "16-64-16 trained sigmoid": (0.9053, 0.9999, 1.0000),
    "16-64-16 spread": (0.8334, 0.9683, 0.9898), "16-64-16 spread sigmoid": (0.9344, 0.9982, 0.9999),
    "16-64-64-16 trained": (0.2177, 0.5852, 0.8468), "16-64-64-16 trained sigmoid": (0.5518, 0.9345, 0.9989),
    "16-64-64-16 spread": (0.6863, 0.9137, 0.9732), "16-64-64-16 spread sigmoid": (0.7700, 0.9549, 0.9950),
    "32-64-16 trained": (0.5086, 0.8449, 0.9494), "32-64-16 trained sigmoid": (0.7647, 0.9940, 1.0000),
    "32-64-16 spread": (0.7669, 0.9451, 0.9824), "32-64-16 spread sigmoid": (0.8714, 0.9907, 0.9995),
    "32-64-64-16 trained": (0.0817, 0.3480, 0.7155), "32-64-64-16 trained sigmoid": (0.2278, 0.6127, 0.9493),
    "32-64-64-16 spread": (0.5715, 0.8517, 0.9527), "32-64-64-16 spread sigmoid": (0.6630, 0.9103, 0.9876),
    "64-64-16 trained": (0.2645, 0.6783, 0.8916), "64-64-16 trained sigmoid": (0.4123, 0.8647, 0.9995),
    "64-64-16 spread": (0.6521, 0.9018, 0.9689), "64-64-16 spread sigmoid": (0.7716, 0.9632, 0.9970),
    "64-64-64-16 trained": (0.0065, 0.0785, 0.4434), "64-64-64-16 trained sigmoid": (0.0847, 0.2938, 0.7075),
    "64-64-64-16 spread": (0.3708, 0.7097, 0.9007), "64-64-64-16 spread sigmoid": (0.4925, 0.7573, 0.9427),
    "density trained": (0.4686, 0.8199, 0.9405), "colour trained": (0.2852, 0.7775, 0.9899),
    "density spread": (0.7686, 0.9459, 0.9826), "colour spread": (0.6566, 0.8997, 0.9846),
}


def _widths(what, res):
    print("%-28s single %.4f   <= 1: %.4f   <= 4: %.4f" % (what, res.single, res.le1, res.le4))
    want = MEASURED_WIDTHS[what]
    for got, m in zip((res.single, res.le1, res.le4), want):
        assert got >= 0.9 * m, (what, got, m)


def test_the_intervals_are_not_vacuous():
    print()
    for n_in, n_hidden in K.CONFIGS:
        for kind in K.WEIGHT_KINDS:
            ref = K.mlp_reference(n_in, n_hidden, kind)
            _widths("%d-%s-16 %s" % (n_in, "-".join(["64"] * n_hidden), kind), F.check(ref.lo, ref.lo, ref.hi))
            _widths("%d-%s-16 %s sigmoid" % (n_in, "-".join(["64"] * n_hidden), kind), F.check(ref.act_lo, ref.act_lo, ref.act_hi))
    for kind in K.FIELD_KINDS:
        ref = K.density_reference(kind)
        _widths("density %s" % kind, F.check(ref.lo, ref.lo, ref.hi))
        # the colour net from pinned h (the emulation's) and the SH interval
        h, _, rgb = field_emulation(kind, "kernel")
        lo, hi = F.colour_intervals(field_ws(kind)[1], K.field_dirs()[:N], h)
        _widths("colour %s" % kind, F.check(lo, lo, hi))
