"""No GPU: the reference of tests/field_backward_reference.py is shown to be sound, to refuse wrong kernels and not to be vacuous, on
the cases of tests/field_backward_cases.py that tests/test_field_backward_exact_gpu.py runs on the device.

  * on the exact nets its point values equal torch float64 autograd of the same network (masks from the f16 activations: on those
    nets every activation is an f16 value, so ReLU's own mask is that mask);
  * the emulation of a launch (plain f32 numpy) lies inside every interval on every interval case at the small counts, under every
    list, and gives the expected values on the exact nets;
  * thirteen wrong kernels, restated as mutations of the emulation, fail the SAME check the GPU test calls (K.check_outputs), each on at
    least one committed case;
  * the intervals are sharp without leaving a sample out: the share of undecided hidden units, the share of dL_din intervals at most
    1 and at most 4 f16 spacings wide and the median dW half-width relative to its mass are printed and held
    to floors that are conditions on the INPUTS, measured from the reference alone."""
import numpy as np
import pytest
import torch

from tests import field_backward_cases as K
from tests import field_backward_reference as B
from tests import field_forward_reference as F


def all_ok(results):
    for r in results:
        assert r.bad == 0, r.worst


def n_bad(results):
    return sum(r.bad for r in results)


# ---------------------------------------------------------------------------------------------------------------- the reference is sound
@pytest.mark.parametrize("n_in,n_hidden", K.CONFIGS)
def test_point_values_equal_float64_autograd_on_exact_nets(n_in, n_hidden):
    n = 300
    blob, x, d = B.exact_backward_net(n_in, n_hidden, n, seed=n_in + n_hidden)
    ws = F.split_weights(blob, n_in, n_hidden)
    for n_out in K.N_OUTS:
        dy = B.pad16(d, n_out)
        tw = [torch.from_numpy(w.astype(np.float64)).requires_grad_(True) for w in ws]
        tx = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
        a = tx
        for w in tw[:-1]:
            a = torch.relu(a @ w.T)
        ((a @ tw[-1].T) * torch.from_numpy(dy.astype(np.float64))).sum().backward()
        din, dw = B.backward_point(ws, x, dy)
        assert np.array_equal(din.astype(np.float64), tx.grad.numpy())
        assert np.array_equal(dw[n], np.concatenate([w.grad.numpy().reshape(-1) for w in tw]))
        assert (dw[n][-(16 - n_out) * F.HID:] == 0).all() or n_out == 16
        # ... and they are inside the intervals, as is the emulation, which gives the expected values too
        ref = B.mlp_backward_intervals(ws, x, None, B.plain_dy(d[:, :n_out], n_out, 0), B.waves(n_in, n_hidden))
        assert F.check(din, ref.din_lo, ref.din_hi).bad == 0 and F.check(dw[n], *ref.dw[n]).bad == 0
        buf, part = B.emulate_backward("plain", ws, x, n, B.waves(n_in, n_hidden), np.ascontiguousarray(d[:, :n_out]), n_out, 0)
        assert np.array_equal(buf.view(np.uint16), din.view(np.uint16)) and np.array_equal(part.astype(np.float64).sum(0), dw[n])


def test_exact_cases_hold_their_condition_at_every_count():
    for n_in, n_hidden in ((32, 1), (32, 2)):
        e = K.exact_case(n_in, n_hidden)
        assert e.n == 2 * B.sweep(e.w) + 33 and sorted(e.want[16][1]) == sorted(K.exact_counts(e.w))
        assert (e.dout[e.n - 33:] != 0).any() and (e.dout[B.sweep(e.w) - 64:B.sweep(e.w) + 64] != 0).any()
    case, want = K.exact_density_case()
    buf, part = B.emulate_backward("density", case.ws, case.inputs, case.n_samples, 8, case.dout, seed=case.seed, scale=case.scale)
    assert np.array_equal(K.rows_of(buf, "density").astype(np.float64), want[0].astype(np.float64))
    assert np.array_equal(part.astype(np.float64).sum(0), want[1][case.n_samples])


# ---------------------------------------------------------------------------------------------------------------- the emulation is inside
@pytest.mark.parametrize("n_in,n_hidden", K.CONFIGS)
def test_emulated_mlp_backward_is_inside_every_interval(n_in, n_hidden):
    w = B.waves(n_in, n_hidden)
    for kind in K.WEIGHT_KINDS:
        for n_out in K.N_OUTS:
            for act in (0, 1):
                case = K.plain_case(n_in, n_hidden, kind, 32 * w + 1, n_out, act)
                for n in K.small_counts(w):
                    all_ok(K.emulate_case(K.prefix(case, n)))


def density_cases():
    n = 257
    for name in ("trained", "spread", "clamp", "underflow"):
        yield K.density_case(name, n)
    for with_dh, with_sigma in ((True, False), (False, True), (False, False)):
        yield K.density_case("trained", n, None, with_dh, with_sigma)
    for lst in K.LISTS:
        yield K.density_case("trained", n, lst)
    yield K.density_case("clamp", n, "subset")


def field_cases():
    n = 129
    for kind in K.WEIGHT_KINDS:
        yield K.field_case(kind, n)
    for lst in K.LISTS:
        yield K.field_case("trained", n, lst)
    yield K.field_case("trained", n, "reversed", 4.0)


def test_emulated_density_backward_is_inside_every_interval():
    for case in density_cases():
        if case.active is None:
            for n in K.small_counts(8):
                all_ok(K.emulate_case(K.prefix(case, n)))
        else:
            all_ok(K.emulate_case(case))


def test_emulated_field_backward_is_inside_every_interval():
    for case in field_cases():
        if case.active is None:
            for n in K.small_counts(4):
                all_ok(K.emulate_case(K.field_prefix(case, n)))
        else:
            all_ok(K.emulate_case(case))
    # the colour net from an ARBITRARY pinned h, then the density net from that launch's own dL/dh: the two-launch form
    c = K.field_case("trained", 129)
    h = K.arbitrary_h(129)
    dh, part_r = B.emulate_backward("colour", c.rws, h, 129, 4, seed=c.rgb, scale=c.scale, dirs=c.dirs)
    ref_c = B.colour_backward_intervals(c.rws, c.dirs, h, None, c.rgb, c.scale)
    all_ok(K.check_outputs(ref_c, 129, dh, part_r, "colour net from a pinned h"))


# ---------------------------------------------------------------------------------------------------------------- wrong kernels are refused
def mutant_cases():
    """The committed cases the mutants are run on: every one is also run on the device."""
    yield K.prefix(K.plain_case(32, 2, "trained", 129, 16, 0), 33)
    yield K.plain_case(32, 2, "trained", 129, 3, 1)
    yield K.prefix(K.density_case("trained", 257), 33)
    yield K.density_case("trained", 257)
    yield K.density_case("clamp", 257)
    yield K.density_case("trained", 257, "reversed")
    yield K.density_case("trained", 257, "subset")
    yield K.field_case("trained", 129, "reversed")
    yield K.field_case("trained", 129, "count33")


def test_every_wrong_kernel_is_refused():
    assert len(B.MUTANTS) == 13
    cases = list(mutant_cases())
    for c in cases:
        all_ok(K.emulate_case(c))
    print()
    for mut in B.MUTANTS:
        caught = [(c.what, n_bad(K.emulate_case(c, mut))) for c in cases]
        caught = [(what, bad) for what, bad in caught if bad]
        print("%-20s refused on %d of %d cases, most outputs outside: %s" % (mut, len(caught), len(cases), max(caught, key=lambda t: t[1]) if caught else "-"))
        assert caught, "the check cannot see the wrong kernel %r: the reference is too wide" % mut


def test_the_one_launch_kernels_own_dw_is_held_by_the_pinned_hand_overs():
    """field_bwd_kernel's weight-gradient code is its own, and the intervals propagated from the features leave a density dW sum room
    of its own size.  A kernel wrong ONLY there (the last partial tile missing from the density net's dW) must fail through the check
    from the pinned dL/dh, on a large share of the 3072 sums, at one sample past a tile and past a workgroup."""
    print()
    for case in (K.field_prefix(K.field_case("trained", 129), 33), K.field_case("trained", 129), K.field_case("trained", 129, "count33")):
        all_ok(K.emulate_case(case))
        res = K.emulate_case(case, "one_launch_density_dw_tail")
        pinned = [r for r in res if r.bad and "density net dW from the pinned dL/dh" in r.worst]
        others = sum(r.bad for r in res) - sum(r.bad for r in pinned)
        print("%s: %d of 3072 density dW sums outside the pinned intervals, %d outputs outside any other" % (case.what, pinned[0].bad if pinned else 0, others))
        assert pinned and pinned[0].bad > 1000


# ---------------------------------------------------------------------------------------------------------------- the intervals are sharp
def stats(ref, n):
    lo, hi = ref.dw[n]
    live = ref.mass > 0
    width = F.ord16(ref.din_hi) - F.ord16(ref.din_lo)
    return (ref.undecided / ref.hidden, float((width <= 1).mean()), float((width <= 4).mean()),
            float(np.median(((hi - lo) / 2)[live] / ref.mass[live])))


def test_the_intervals_are_sharp_and_no_sample_is_left_out():
    """Measured from the reference alone, on the trained-like weights at n = 4096 with n_out = 16.  The floors
    are conditions on the inputs: how much room the unknown summation order and the undecided masks get."""
    n = 4096
    print()
    for n_in, n_hidden in K.CONFIGS:
        und, le1, le4, dw = stats(K.plain_case(n_in, n_hidden, "trained", n, 16, 0).ref, n)
        print("mlp %d-%d: undecided %.1e of the hidden units; dL_din <= 1 spacing %.3f, <= 4 spacings %.3f; dW half-width / mass median %.1e" % (
            n_in, n_hidden, und, le1, le4, dw))
        # (the dW half-width is B = (n + W) 2^-23 mass plus the spread of the corners: the spread may be three times B)
        assert und < 1e-3 and le1 > 0.5 and le4 > 0.8 and dw < 4 * (n + 8) * B.U23
    # The one-launch field, everything propagated from the features through eight layers, is NOT sharp: every h is an interval, the
    # colour net's forward and backward widen it by the cancellation of each sum (mass / |sum|) and dL/dh reaches the density net
    # wide.  Its figures are printed, not held to a floor; what pins the one-launch kernel is its bit equality with the two-launch
    # chain, whose halves are held to intervals from PINNED hand-overs (the launch's own h and dL/dh), printed next.
    fc = K.field_case("trained", n)
    for name, ref in zip(("density net (one launch, dL/dh an interval)", "colour net (one launch, h an interval)"), fc.ref):
        und, le1, le4, dw = stats(ref, n)
        print("%s: undecided %.1e; din <= 1 spacing %.3f, <= 4 spacings %.3f; dW half-width / mass median %.1e" % (name, und, le1, le4, dw))
        assert und < 1e-2
    und, le1, le4, dw = stats(B.colour_backward_intervals(fc.rws, fc.dirs, K.arbitrary_h(n), None, fc.rgb, fc.scale, [n]), n)
    print("colour net from a pinned h: undecided %.1e; dL/dh <= 1 spacing %.3f, <= 4 spacings %.3f, dW half-width / mass median %.1e" % (und, le1, le4, dw))
    assert und < 1e-3 and le4 > 0.25
    dc = K.density_case("trained", n)
    und, le1, le4, dw = stats(dc.ref, n)
    print("density net from a pinned dL/dh: undecided %.1e; dfeats <= 1 spacing %.3f, <= 4 spacings %.3f; dW half-width / mass median %.1e" % (und, le1, le4, dw))
    assert und < 1e-3 and le1 > 0.5 and le4 > 0.8
