"""ngp_mlp_bwd, ngp_density_bwd, ngp_field_bwd_two_launches, ngp_field_bwd and ngp_field_bwd_guarded against the interval reference of
tests/field_backward_reference.py (its docstring has the contract, the undecided ReLU masks, the model and every derivation).

Every output buffer is prefilled with a NaN bit pattern and carries a guard band: every element that should be written must be inside
its interval (a NaN is outside every interval), nothing behind the outputs nor at a compact position >= n_eff may change, every
partial row must be finite, and dW is the float64 sum of ALL partial rows, so the reference knows nothing of tiles and workgroups.  No
sample is filtered out: a hidden unit whose forward interval cannot decide its mask gets the hull of both outcomes.
tests/test_field_backward_reference_cpu.py shows on the same cases, without a GPU, that thirteen wrong kernels fail the checks used here
(K.check_outputs, K.check_field_outputs) and how narrow the intervals are.

  * ngp_mlp_bwd: six instantiations x n_out 1 / 3 / 8 / 16 x out_act 0 / 1.  Exact nets (act 0) at 1, 31, 32, 33, 32 W - 1, 32 W,
    32 W + 1, sweep - 1, sweep, sweep + 1 and 2 sweeps + 33 samples (W waves per workgroup, sweep = 256 W 32): dL_din bit for bit, dW
    equal to the expected sums.  Trained-like and wide-spread weights at the counts up to 32 W + 1 (and sweep + 33 for 32-64-64):
    intervals.  The padded rows of dWo are exactly zero in every partial row; dL_din = NULL is accepted.
  * ngp_density_bwd with and without each of dL_dh and dL_dsigmas, with and without lists, on the clamp edges of the TruncExp
    backward, on a net whose positive pre-activations underflow in f16, and on an exact net with h0 = 0.
  * ngp_field_bwd_two_launches from an ARBITRARY h: dh_scratch inside the colour net's interval, the density half inside intervals
    propagated from the launch's OWN dh_scratch.
  * ngp_field_bwd / ngp_field_bwd_guarded (device-side loss-scale factor 4) at every count and under every list: dfeats bit for bit
    the two-launch chain fed the forward's own h; both dW blobs (the one-launch kernel's own weight-gradient code) inside the
    intervals from the PINNED hand-overs, that h and that chain's dh_scratch; dfeats and both dW blobs also inside the (wide)
    intervals propagated from the features; positions >= n_eff untouched, *n_active = 0 gives all-zero partial rows, h and
    dh_scratch are not touched.
  * the element the finding below was worked out on, as a case of its own.

THE FIRST RUN on an MI355X (DESIGN.md section 25 has the figures).  No kernel code changed.  With the mass of the forward reference,
sum |w| |a|, three of the 38 tests stopped at an output outside (one dL_din value, three dW sums), all on the wide-spread weights, whose
small entries and hidden gradients are f16 subnormals: the matrix unit aligns a product by its operands' exponent fields and does not
normalise a subnormal, so its 2^-23 is relative to max(|v|, 2^-14).  The model was corrected by that derivation (the reference's
docstring, SUBNORMAL OPERANDS); since then 0 outputs are outside, all exact cases are bit-equal, the largest dW error beyond the
corners is 0.017 of its bound B (0.027 of the true-mass bound on the trained-like weights, 9.9 on the wide-spread ones), and single
backward layers from pinned operands use at most 0.0056 of e (64 terms).  Intervals: 1e-5 .. 1e-4 of the hidden units undecided, 64 - 93 %
of the dL_din intervals at most one f16 spacing wide, 87 - 98 % at most four."""
import numpy as np
import pytest
import torch

from tests import field_backward_cases as K
from tests import field_backward_reference as B
from tests import field_forward_cases as FK
from tests import field_forward_reference as F

pytestmark = pytest.mark.gpu

PREFILL16, PREFILL32 = 0x7E5A, 0x7FC5A5A5      # NaN bit patterns (f16, f32)
GUARD = 4096


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from ngp_pl_amd import _lib
    return _lib


def up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def buf16(numel):
    return torch.full((numel + GUARD,), PREFILL16, dtype=torch.int16, device="cuda")


def buf32(numel):
    return torch.full((numel + GUARD,), PREFILL32, dtype=torch.int32, device="cuda")


def take(buf, numel, shape):
    """The host copy of a prefilled buffer's first numel values as f16 / f32; asserts that nothing behind them changed."""
    host = buf.cpu().numpy()
    pre, ft = (PREFILL16, np.float16) if host.dtype == np.int16 else (PREFILL32, np.float32)
    assert (host[numel:] == pre).all(), "%d values written behind the first %d" % (int((host[numel:] != pre).sum()), numel)
    return host[:numel].view(ft).reshape(shape)


def all_ok(results):
    for r in results:
        assert r.bad == 0, r.worst


def rows_finite(part, what):
    assert np.isfinite(part).all(), "%s: %d values of the partial rows are not finite (unwritten?)" % (what, int((~np.isfinite(part)).sum()))


# ---------------------------------------------------------------------------------------------------------------- ngp_mlp_bwd
def run_mlp_bwd(lib, x, w, dout, n_in, n_hidden, n_out, act, n, with_din=True):
    n_part, size = lib.call("ngp_mlp_bwd_partials", n), B.net_size(n_in, n_hidden)
    assert n_part == B.partials(n)
    assert x.shape == (x.shape[0], n_in) and x.shape[0] >= n and dout.shape == (dout.shape[0], n_out) and dout.shape[0] >= n and w.numel() == size
    din, part = (buf16(n * n_in) if with_din else None), buf32(n_part * size)
    lib.call("ngp_mlp_bwd", lib.ptr(x), lib.ptr(w), lib.ptr(dout), n_in, n_hidden, n_out, act, n, lib.ptr(din), lib.ptr(part), lib.stream())
    torch.cuda.synchronize()
    return (take(din, n * n_in, (n, n_in)) if with_din else None), take(part, n_part * size, (n_part, size))


@pytest.mark.parametrize("n_in,n_hidden", K.CONFIGS)
def test_mlp_backward_exact_nets(lib, n_in, n_hidden):
    """Bit equality of dL_din and equality of the summed dW with the ONE expected value, at every count around the tile, the
    workgroup and the sweep of the capped launch."""
    e = K.exact_case(n_in, n_hidden)
    x, w = up(e.x), up(e.blob)
    size = B.net_size(n_in, n_hidden)
    for n_out in K.N_OUTS:
        dout = up(e.dout[:, :n_out])
        want_din, want_dw = e.want[n_out]
        for n in K.exact_counts(e.w):
            what = "exact net %d-%d n_out=%d n=%d" % (n_in, n_hidden, n_out, n)
            din, part = run_mlp_bwd(lib, x, w, dout, n_in, n_hidden, n_out, 0, n)
            bad = din.view(np.uint16) != want_din[:n].view(np.uint16)
            assert not bad.any(), "%s: %d values of dL_din differ, first at %s" % (what, int(bad.sum()), np.argwhere(bad)[0])
            rows_finite(part, what)
            bad = part.astype(np.float64).sum(0) != want_dw[n]
            assert not bad.any(), "%s: %d sums of dW differ, first at %s" % (what, int(bad.sum()), np.argwhere(bad)[0])
            assert (part[:, size - (16 - n_out) * F.HID:] == 0).all(), what + ": a padded row of dWo is not zero"
        n = 32 * e.w + 1
        _, part = run_mlp_bwd(lib, x, w, dout, n_in, n_hidden, n_out, 0, n, with_din=False)          # dL_din = NULL
        assert np.array_equal(part.astype(np.float64).sum(0), want_dw[n]), "dW without dL_din"


def check_plain(lib, case, x, w, dout, n):
    c = K.prefix(case, n)
    din, part = run_mlp_bwd(lib, x, w, dout, case.n_in, case.n_hidden, case.n_out, case.out_act, n)
    rows_finite(part, c.what)
    all_ok(K.check_outputs(c.ref, n, din, part, c.what))
    size = part.shape[1]
    assert (part[:, size - (16 - case.n_out) * F.HID:] == 0).all(), c.what + ": a padded row of dWo is not zero"


@pytest.mark.parametrize("n_in,n_hidden", K.CONFIGS)
def test_mlp_backward_inside_every_interval(lib, n_in, n_hidden):
    w_ = B.waves(n_in, n_hidden)
    for kind in K.WEIGHT_KINDS:
        w = up(FK.weights(n_in, n_hidden, kind))
        for n_out in K.N_OUTS:
            for act in (0, 1):
                case = K.plain_case(n_in, n_hidden, kind, 32 * w_ + 1, n_out, act)
                x, dout = up(case.inputs), up(case.dout)
                for n in K.small_counts(w_):
                    check_plain(lib, case, x, w, dout, n)
    if (n_in, n_hidden) == (32, 2):                      # one instantiation crosses the sweep
        n = B.sweep(w_) + 33
        for n_out, act in ((3, 1), (16, 0)):
            case = K.plain_case(n_in, n_hidden, "trained", n, n_out, act)
            check_plain(lib, case, up(case.inputs), up(FK.weights(n_in, n_hidden, "trained")), up(case.dout), n)


@pytest.mark.parametrize("n_in", (16, 32, 64))
def test_single_layer_input_gradient_error_to_limit(lib, n_in):
    """One dense accumulation from pinned operands: a 1-hidden-layer net whose output layer is a 0/1 selection (hidden unit k takes
    dL_dout[k mod 16] exactly), so dL_din = f16(W0^T dh0) with dh0 known wherever the mask is decided.  The accumulator is not
    observable; printed (and held below 1) is the smallest |a - s| / e over the accumulators a that round to the output."""
    n = 4099
    W0 = K.ws_of(n_in, 1, "trained")[0]
    Wo = np.zeros((16, F.HID), np.float16)
    Wo[np.arange(F.HID) % 16, np.arange(F.HID)] = 1
    blob = np.concatenate([W0.reshape(-1), Wo.reshape(-1)])
    x, d = FK.inputs(n_in)[:n], K.dout(n, 5)
    ref = B.mlp_backward_intervals([W0, Wo], x, None, B.plain_dy(d, 16, 0), B.waves(n_in, 1))
    din, part = run_mlp_bwd(lib, up(x), up(blob), up(d), n_in, 1, 16, 0, n)
    all_ok(K.check_outputs(ref, n, din, part, "single layer K=64 into %d inputs" % n_in))
    acts, _, _ = B.forward_intervals([W0, Wo], x, None)
    decided = ((acts[1][0] > 0) | (acts[1][1] == 0)).all(axis=1)
    dh0 = np.where(acts[1][0] > 0, np.tile(d.astype(np.float64), (1, 4)), 0.0)
    s, _, e = F.layer_interval(W0.T, dh0, dh0)
    live = decided[:, None] & (e > 0)
    worst = float(F.least_ratio(din, s, e)[live].max())
    print("\nsingle backward layer, 64 terms into %d inputs: worst least |a - s| / e = %.4f over %d samples with every mask decided of %d" % (
        n_in, worst, int(decided.sum()), n))
    assert worst <= 1.0


def test_subnormal_operands_are_aligned_by_their_exponent_field(lib):
    """The element the finding of the reference's docstring (SUBNORMAL OPERANDS) was worked out on, kept as a case: dW0[34, 22] of
    64-64-16 on the wide-spread weights at n = 31, n_out = 1, is ten products dh0 * x with dh0 in {1..4} * 2^-24, every operand
    pinned.  Asserted without the device: the exact sum is 552.109375 * 2^-34, and 552 * 2^-34, what the first run returned, is
    refused by the bound from the TRUE mass, (n + W) 2^-23 sum |dh0| |x|.  Asserted on the device: the sum is inside the interval
    from the nominal mass.  The device's value is printed."""
    n, row, col = 31, 34, 22
    case = K.prefix(K.plain_case(64, 1, "spread", 129, 1, 0), n)
    W0, Wo = [m.astype(np.float64) for m in case.ws]
    x, d = case.inputs.astype(np.float64), case.dout.astype(np.float64)
    on = F.f16(x @ W0.T) > 0
    dh0 = np.where(on[:, row], F.f16(d[:, 0] * Wo[0, row]).astype(np.float64), 0.0)
    live = dh0 != 0
    assert live.sum() == 10 and (np.abs(dh0[live]) < 2.0 ** -14).all() and set(np.abs(dh0[live]) * 2.0 ** 24) <= {1.0, 2.0, 3.0, 4.0}
    products = dh0 * x[:, col]
    exact = products.sum()
    assert exact == 552.109375 * 2.0 ** -34
    true_mass_bound = (n + 4) * B.U23 * np.abs(products).sum()
    assert abs(552.0 * 2.0 ** -34 - exact) > true_mass_bound
    din, part = run_mlp_bwd(lib, up(case.inputs), up(case.blob), up(case.dout), 64, 1, 1, 0, n)
    all_ok(K.check_outputs(case.ref, n, din, part, case.what))
    got = float(part.astype(np.float64).sum(0)[row * 64 + col])
    lo, hi = case.ref.dw[n]
    print("\ndW0[%d, %d]: exact %.6f * 2^-34, device %.6f * 2^-34, |device - exact| = %.2f of the true-mass bound; interval from the nominal mass [%.1f, %.1f] * 2^-34" % (
        row, col, exact * 2.0 ** 34, got * 2.0 ** 34, abs(got - exact) / true_mass_bound, lo[row * 64 + col] * 2.0 ** 34, hi[row * 64 + col] * 2.0 ** 34))


# ---------------------------------------------------------------------------------------------------------------- ngp_density_bwd
def list_dev(case):
    if case.active is None:
        return None, None
    return up(case.active), torch.tensor([case.n_active], dtype=torch.int32, device="cuda")


def run_density_bwd(lib, case, n=None):
    n = case.n_samples if n is None else n
    n_part = lib.call("ngp_field_bwd_partials", n)
    assert n_part == B.partials(n)
    assert case.inputs.shape[0] >= n and case.blob.size == 3072 and (case.dout is None or case.dout.shape[0] >= n)
    assert (case.seed is None or case.seed.shape[0] >= n) and (case.active is None or case.active.size > min(case.n_active, n))
    dfeats, part = buf16(32 * n), buf32(n_part * 3072)
    feats, w = up(FK.level_major(case.inputs[:n])), up(case.blob)
    dh, sig = up(None if case.dout is None else case.dout[:n]), up(None if case.seed is None else case.seed[:n])
    active, n_active = list_dev(case)
    lib.call("ngp_density_bwd", lib.ptr(feats), lib.ptr(w), lib.ptr(dh), lib.ptr(sig), K.LOSS_SCALE, n, lib.ptr(active), lib.ptr(n_active),
             lib.ptr(dfeats), lib.ptr(part), lib.stream())
    torch.cuda.synchronize()
    return take(dfeats, 32 * n, (16, n, 2)), take(part, n_part * 3072, (n_part, 3072))


def check_density(lib, case):
    dfeats, part = run_density_bwd(lib, case)
    rows_finite(part, case.what)
    all_ok(K.check_outputs(case.ref, case.n_eff, K.rows_of(dfeats, "density"), part, case.what))


@pytest.mark.parametrize("name", ("trained", "spread", "clamp", "underflow"))
def test_density_backward_inside_every_interval(lib, name):
    case = K.density_case(name, 257)
    for n in K.small_counts(8):
        check_density(lib, K.prefix(case, n))
    if name == "trained":
        for with_dh, with_sigma in ((True, False), (False, True), (False, False)):
            check_density(lib, K.density_case(name, 257, None, with_dh, with_sigma))
        check_density(lib, K.density_case(name, B.sweep(8) + 33))
    if name == "clamp":
        check_density(lib, K.density_case(name, 257, "subset"))


@pytest.mark.parametrize("lst", K.LISTS)
def test_density_backward_over_a_list(lib, lst):
    check_density(lib, K.density_case("trained", 257, lst))
    check_density(lib, K.density_case("trained", 257, lst, True, False))


def test_density_backward_exact_net_with_h0_zero(lib):
    case, (want_din, want_dw) = K.exact_density_case()
    for n in K.small_counts(8):
        dfeats, part = run_density_bwd(lib, case, n)
        got = K.rows_of(dfeats, "density")
        bad = got.view(np.uint16) != want_din[:n].view(np.uint16)
        assert not bad.any(), "exact density net n=%d: %d values of dfeats differ, first at %s" % (n, int(bad.sum()), np.argwhere(bad)[0])
        rows_finite(part, "exact density net")
        assert np.array_equal(part.astype(np.float64).sum(0), want_dw[n]), "exact density net n=%d: dW" % n


# ---------------------------------------------------------------------------------------------------------------- the field
def run_field_bwd(lib, case, entry, h=None):
    """entry: "one" (ngp_field_bwd), "guarded" (ngp_field_bwd_guarded, the device-side factor) or "two" (ngp_field_bwd_two_launches,
    which has no device-side factor: it gets the product as its loss scale).  Returns dfeats (16, n, 2), density rows, colour rows,
    dh_scratch (n, 16), all as written over the prefill."""
    n = case.n_samples
    n_part = lib.call("ngp_field_bwd_partials", n)
    assert n_part == B.partials(n)
    assert case.feats.shape == (n, 32) and case.dirs.shape == (n, 3) and case.sig.shape == (n,) and case.rgb.shape == (n, 3)
    assert (h is None or h.shape == (n, 16)) and (case.active is None or case.active.size > min(case.n_active, n))
    dfeats, dh, part = buf16(32 * n), buf16(16 * n), buf32(n_part * 10240)
    feats, dirs, dw, rw = up(FK.level_major(case.feats)), up(case.dirs), up(case.dw), up(case.rw)
    sig, rgb, h_d = up(case.sig), up(case.rgb), up(h)
    active, n_active = list_dev(case)
    if entry == "guarded":
        dev = torch.tensor([1.0 if case.dev_scale is None else case.dev_scale], dtype=torch.float32, device="cuda")
        lib.call("ngp_field_bwd_guarded", lib.ptr(feats), lib.ptr(dirs), lib.ptr(h_d), lib.ptr(dw), lib.ptr(rw), lib.ptr(sig), lib.ptr(rgb), K.LOSS_SCALE,
                 lib.ptr(dev), 0.0, n, lib.ptr(active), lib.ptr(n_active), lib.ptr(dh), lib.ptr(dfeats), lib.ptr(part), None, 0, lib.stream())
    else:
        assert entry == "two" or case.dev_scale is None
        lib.call("ngp_field_bwd" if entry == "one" else "ngp_field_bwd_two_launches", lib.ptr(feats), lib.ptr(dirs), lib.ptr(h_d), lib.ptr(dw),
                 lib.ptr(rw), lib.ptr(sig), lib.ptr(rgb), case.scale, n, lib.ptr(active), lib.ptr(n_active), lib.ptr(dh), lib.ptr(dfeats),
                 lib.ptr(part), lib.stream())
    torch.cuda.synchronize()
    rows = take(part, n_part * 10240, (n_part * 10240,))
    return (take(dfeats, 32 * n, (16, n, 2)), rows[:n_part * 3072].reshape(n_part, 3072), rows[n_part * 3072:].reshape(n_part, 7168),
            take(dh, 16 * n, (n, 16)))


def forward_h(lib, case):
    n = case.n_samples
    h, sig, rgb = torch.empty(n, 16, dtype=torch.float16, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, 3, device="cuda")
    feats, dirs, dw, rw = up(FK.level_major(case.feats)), up(case.dirs), up(case.dw), up(case.rw)
    lib.call("ngp_field_fwd", lib.ptr(feats), lib.ptr(dirs), lib.ptr(dw), lib.ptr(rw), n, lib.ptr(sig), lib.ptr(rgb), lib.ptr(h), lib.stream())
    torch.cuda.synchronize()
    return h.cpu().numpy()


def check_two_launches(lib, case, h, what):
    """dh_scratch inside the colour net's interval from the pinned h; the density half from the launch's OWN dh_scratch.  Returns
    dfeats, dh_scratch and the colour net's intervals."""
    dfeats, part_d, part_r, dh = run_field_bwd(lib, case, "two", h)
    rows_finite(part_d, what)
    rows_finite(part_r, what)
    n_eff, ids = case.n_eff, case.ids
    if n_eff == 0:
        assert (part_d == 0).all() and (part_r == 0).all() and K.untouched(dh) and K.untouched(dfeats), what + ": an empty launch wrote something"
        return dfeats, dh, None
    ref_c = B.colour_backward_intervals(case.rws, case.dirs[ids], h[ids], None, case.rgb[ids], case.scale, [n_eff])
    all_ok(K.check_outputs(ref_c, n_eff, dh, part_r, what + " colour net"))
    ref_d = B.density_backward_intervals(case.dws, case.feats[ids], dh[:n_eff], None, case.sig[ids], case.scale, 8, [n_eff])
    all_ok(K.check_outputs(ref_d, n_eff, K.rows_of(dfeats, "field"), part_d, what + " density net from its own dL/dh"))
    return dfeats, dh, ref_c


def check_field(lib, case, entry="one"):
    """The one-launch kernel.  Its dfeats is bit for bit that of the two-launch chain fed the forward's own h, so its hand-overs ARE
    that h and that chain's dh_scratch: both dW blobs (its own weight-gradient code) are held to the intervals from those pinned
    hand-overs, next to the wide ones propagated from the features (K.check_field_outputs)."""
    dfeats, part_d, part_r, dh = run_field_bwd(lib, case, entry)
    rows_finite(part_d, case.what)
    rows_finite(part_r, case.what)
    assert K.untouched(dh), case.what + ": the one-launch kernel wrote dh_scratch"
    if case.n_eff == 0:
        assert (part_d == 0).all() and (part_r == 0).all()
    h = forward_h(lib, case)
    two, two_dh, pin_c = check_two_launches(lib, case, h, case.what + " two launches from the forward's h")
    assert np.array_equal(dfeats.view(np.uint16), two.view(np.uint16)), "%s: dfeats differs from the two-launch chain in %d values" % (
        case.what, int((dfeats.view(np.uint16) != two.view(np.uint16)).sum()))
    all_ok(K.check_field_outputs(case, dfeats, part_d, part_r, h, two_dh, pin_c))
    return dfeats


@pytest.mark.parametrize("kind", K.WEIGHT_KINDS)
def test_field_backward_at_every_count(lib, kind):
    case, scaled = K.field_case(kind, 129), K.field_case(kind, 129, None, 4.0)
    for n in K.small_counts(4):
        c = K.field_prefix(case, n)
        check_field(lib, c)
        check_field(lib, K.field_prefix(scaled, n), "guarded")           # loss_scale_dev = 4
        check_two_launches(lib, c, K.arbitrary_h(129)[:n], c.what + " two launches from an arbitrary h")


@pytest.mark.parametrize("entry", ("one", "guarded"))
def test_field_backward_across_the_sweep(lib, entry):
    check_field(lib, K.field_case("trained", B.sweep(4) + 33, None, 4.0 if entry == "guarded" else None), entry)


@pytest.mark.parametrize("lst", K.LISTS)
def test_field_backward_over_a_list(lib, lst):
    case = K.field_case("trained", 129, lst)
    one = check_field(lib, case)
    guarded = check_field(lib, case, "guarded")                         # no device factor: the same launch
    assert np.array_equal(one.view(np.uint16), guarded.view(np.uint16))
    check_two_launches(lib, case, K.arbitrary_h(129), case.what + " two launches from an arbitrary h")
    check_field(lib, K.field_case("trained", 129, lst, 4.0), "guarded")  # loss_scale_dev = 4
