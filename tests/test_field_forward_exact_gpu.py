"""ngp_mlp_fwd, ngp_field_fwd (+ _n, _list), ngp_density_fwd (+ _scatter) against the interval reference of
tests/field_forward_reference.py (its docstring has the model, e = K * 2^-23 * mass per layer, and every derivation).

Every output buffer is prefilled with a NaN bit pattern and carries a guard band: every element that should be written must be inside
its interval (a NaN is outside every interval), and nothing behind the n outputs, nor any sample a list or a device count leaves out,
may change.  No output is filtered out.  tests/test_field_forward_reference_cpu.py shows on the same cases, without a GPU, that nine
wrong kernels fail the check function used here (F.check) and how narrow the intervals are.

  * ngp_mlp_fwd: six instantiations x n_out 1 / 3 / 8 / 16 (row length n_out) x out_act 0 / 1 x twelve counts around the 32-sample
    tile, the 128-sample workgroup and the 65 536-sample sweep of the capped launch, trained-like and wide-spread weights: intervals.
    Exact nets and one-hot inputs (every (j, k) of every matrix): bit equality.
  * ngp_field_fwd at every count: h inside the interval from the features, sigma against the kernel's own h[0], rgb inside the
    interval propagated from the kernel's own h, rgb an f16 value; the h[0] edges of sigma (+-11, overflow from 89, zero from -104).
  * the variants of one computation, bit for bit, at counts that cross 65 536: without h_out, ngp_density_fwd, ngp_field_fwd_n with a
    launch bound several sweeps above the device count, ngp_field_fwd_list (more than 65 536 entries, -1 padding, ids >= stride, a
    device count inside the list, a padded entry last in a sweep), ngp_density_fwd_scatter (repeated targets across sweeps, twice).

THE FIRST RUN on an MI355X (DESIGN.md section 19 has the figures).  No output was outside its interval.  The single-layer cases used at
most 0.020 (K = 16), 0.0058 (K = 32) and 0.0027 (K = 64) of e; exact nets and one-hot inputs were bit-equal.  The k-ordered f32 chain
reproduced 99.4 - 99.9 % of the outputs in each of its three K orders and 100 % in none, on any case: the MFMA is not such a chain,
NO emulation is pinned (PIN_EMULATED = None) and the interval stands alone.  The shares are still printed.  For h0 between -104 and
-87.34 the device returns a flushed zero, never a subnormal."""
import numpy as np
import pytest
import torch

from tests import field_forward_cases as K
from tests import field_forward_reference as F

pytestmark = pytest.mark.gpu

# The emulation order ("asc", "desc", "kernel") that reproduced 100 % of the outputs on every case of the first run: equality with it
# would be asserted next to the interval, as tests/test_hashgrid_forward_exact_gpu.py does.  None did.
PIN_EMULATED = None

PREFILL16, PREFILL32 = 0x7E5A, 0x7FC5A5A5      # NaN bit patterns (f16, f32)
GUARD = 4096
_DEV = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from ngp_pl_amd import _lib
    return _lib


def dev(key, make):
    if key not in _DEV:
        _DEV[key] = torch.from_numpy(np.ascontiguousarray(make())).cuda()
    return _DEV[key]


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def buf16(numel):
    return torch.full((numel + GUARD,), PREFILL16, dtype=torch.int16, device="cuda")


def buf32(numel):
    return torch.full((numel + GUARD,), PREFILL32, dtype=torch.int32, device="cuda")


def take(buf, rows, cols, written_rows=None):
    """The host copy of a prefilled buffer as (rows, cols) f16 / f32; asserts that nothing behind written_rows x cols values changed."""
    host = buf.cpu().numpy()
    pre, ft = (PREFILL16, np.float16) if host.dtype == np.int16 else (PREFILL32, np.float32)
    m = (rows if written_rows is None else written_rows) * cols
    assert (host[m:] == pre).all(), "%d values written behind the first %d" % (int((host[m:] != pre).sum()), m)
    return host[:rows * cols].view(ft).reshape(rows, cols)


def ok(res):
    assert res.bad == 0, res.worst


def equal_bits(a, b, what):
    ia, ib = a.view(np.int16 if a.dtype == np.float16 else np.int32), b.view(np.int16 if b.dtype == np.float16 else np.int32)
    assert a.shape == b.shape and np.array_equal(ia, ib), "%s: %d of %d values differ" % (what, int((ia != ib).sum()), ia.size)


def same_value_share(got16, emu16):
    return float((got16.astype(np.float32) == emu16.astype(np.float32)).mean())


# ---------------------------------------------------------------------------------------------------------------- ngp_mlp_fwd
def run_mlp(lib, x, w, n_in, n_hidden, n_out, act, n):
    out = buf16(n * n_out)
    lib.call("ngp_mlp_fwd", lib.ptr(x), lib.ptr(w), n_in, n_hidden, n_out, act, n, lib.ptr(out), lib.stream())
    torch.cuda.synchronize()
    return take(out, n, n_out)


@pytest.mark.parametrize("n_in,n_hidden", K.CONFIGS)
def test_mlp_inside_every_interval(lib, n_in, n_hidden):
    print()
    for kind in K.WEIGHT_KINDS:
        ref = K.mlp_reference(n_in, n_hidden, kind)
        x = dev(("x", n_in), lambda: K.inputs(n_in))
        w = up(K.weights(n_in, n_hidden, kind))
        for n in K.COUNTS:
            for n_out in K.N_OUTS:
                for act in (0, 1):
                    got = run_mlp(lib, x, w, n_in, n_hidden, n_out, act, n)
                    lo, hi = (ref.act_lo, ref.act_hi) if act else (ref.lo, ref.hi)
                    ok(F.check(got, lo[:n, :n_out], hi[:n, :n_out], "mlp %d-%d %s n=%d n_out=%d act=%d" % (n_in, n_hidden, kind, n, n_out, act)))
        # the first-run report: the share of outputs equal to each emulation order, at a count that crosses the sweep
        n = 65536 + 129
        rows = K.emulation_rows(n)
        got = run_mlp(lib, x, w, n_in, n_hidden, 16, 0, n)[rows]
        ws = F.split_weights(K.weights(n_in, n_hidden, kind), n_in, n_hidden)
        shares = {o: same_value_share(got, F.emulate_mlp(ws, K.inputs(n_in)[rows], o)) for o in F.ORDERS}
        print("mlp %d-%d %-8s equal to the emulation: %s" % (n_in, n_hidden, kind, "  ".join("%s %.4f" % (o, shares[o]) for o in F.ORDERS)))
        if PIN_EMULATED:
            assert shares[PIN_EMULATED] == 1.0


@pytest.mark.parametrize("n_in,n_hidden", K.CONFIGS)
def test_mlp_exact_nets_and_one_hot_inputs(lib, n_in, n_hidden):
    """Bit equality, the sign of a zero included (a tiny negative product of the output layer rounds to -0, ReLU gives +0): dense
    integer nets in which any summation order gives the same bits, and one-hot inputs, where every output is ONE product f16(w_jk v)."""
    n = 4099
    blob, x, want = F.exact_net(n_in, n_hidden, n, seed=n_in + n_hidden)
    for n_out in K.N_OUTS:
        got = run_mlp(lib, up(x), up(blob), n_in, n_hidden, n_out, 0, n)
        equal_bits(got, np.ascontiguousarray(want[:, :n_out]), "exact net %d-%d n_out=%d" % (n_in, n_hidden, n_out))
    cases = 0
    for name, blob, x, want in K.one_hot_cases(n_in, n_hidden):
        got = run_mlp(lib, up(x), up(blob), n_in, n_hidden, 16, 0, x.shape[0])
        bad = got.view(np.int16) != want.view(np.int16)
        assert not bad.any(), "one-hot %d-%d %s: %d outputs differ, first at %s" % (n_in, n_hidden, name, int(bad.sum()), np.argwhere(bad)[0])
        cases += 1
    assert cases == 4 + (F.HID // n_in) * (1 + 4 * (n_hidden == 2))          # W0 in four blocks; per shift Wo, and W1 in four blocks


@pytest.mark.parametrize("n_in,n_hidden", K.CONFIGS)
def test_single_layer_error_to_limit(lib, n_in, n_hidden):
    """One dense layer from pinned inputs, shown through identity / selection matrices: the output is relu(f16(accumulator)).  The
    accumulator is not observable; printed (and held below 1) is the smallest |a - s| / e over the accumulators a that round to the
    output, over the outputs that ReLU lets through."""
    worst, off_nearest = 0.0, 0
    for block in range(4):
        blob, x, s, e = K.passthrough_case(n_in, n_hidden, block)
        got = run_mlp(lib, up(x), up(blob), n_in, n_hidden, 16, 0, x.shape[0])
        ok(F.check(got, np.maximum(F.f16(s - e), np.float16(0)), np.maximum(F.f16(s + e), np.float16(0)), "single layer %d-%d block %d" % (n_in, n_hidden, block)))
        live = s > e
        worst = max(worst, float(F.least_ratio(got, s, e)[live].max()))
        off_nearest += int((got.astype(np.float32) != np.maximum(F.f16(s), np.float16(0)).astype(np.float32)).sum())
    print("\nsingle layer K=%d (%d hidden): worst least |a - s| / e = %.4f; outputs that are not f16(s): %d" % (n_in, n_hidden, worst, off_nearest))
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------- the field
def field_dev(kind):
    dw, rw = K.field_weights(kind)
    return dev(("dw", kind), lambda: dw), dev(("rw", kind), lambda: rw)


def feats_dev(n):
    return dev(("feats", n), lambda: K.level_major(K.field_feats()[:n]))


def dirs_dev():
    return dev(("dirs",), lambda: K.field_dirs())


def run_field(lib, feats, dirs, dw, rw, n, with_h=True, count=None, bound=None, lst=None, n_list_max=None, rows=None):
    """ngp_field_fwd / _n (bound, count) / _list (lst, n_list_max, count).  Returns h (rows, 16) f16 or None, sigma (rows,) f32, rgb
    (rows, 3) f32 as written over the prefill; rows: the size of the output buffers (n, or the launch bound)."""
    rows = (n if bound is None else bound) if rows is None else rows
    h, sig, rgb = (buf16(rows * 16) if with_h else None), buf32(rows), buf32(rows * 3)
    n_dev = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    if lst is not None:
        lib.call("ngp_field_fwd_list", lib.ptr(feats), lib.ptr(dirs), lib.ptr(dw), lib.ptr(rw), n, lib.ptr(lst), n_list_max, lib.ptr(n_dev),
                 lib.ptr(sig), lib.ptr(rgb), lib.ptr(h), lib.stream())
    elif bound is not None:
        lib.call("ngp_field_fwd_n", lib.ptr(feats), lib.ptr(dirs), lib.ptr(dw), lib.ptr(rw), bound, lib.ptr(n_dev), lib.ptr(sig), lib.ptr(rgb),
                 lib.ptr(h), lib.stream())
    else:
        lib.call("ngp_field_fwd", lib.ptr(feats), lib.ptr(dirs), lib.ptr(dw), lib.ptr(rw), n, lib.ptr(sig), lib.ptr(rgb), lib.ptr(h), lib.stream())
    torch.cuda.synchronize()
    return (take(h, rows, 16) if with_h else None), take(sig, rows, 1)[:, 0], take(rgb, rows, 3)


@pytest.mark.parametrize("kind", K.FIELD_KINDS)
def test_field_inside_every_interval(lib, kind):
    dw, rw = field_dev(kind)
    print()
    for n in K.COUNTS:
        h, sig, rgb = run_field(lib, feats_dev(n), dirs_dev(), dw, rw, n)
        for res in K.check_field(kind, np.arange(n), h, sig, rgb, "field %s n=%d" % (kind, n)):
            ok(res)
    n = 65536 + 129
    rows = K.emulation_rows(n)
    h, sig, rgb = run_field(lib, feats_dev(n), dirs_dev(), dw, rw, n)
    dws, rws = [F.split_weights(b, 32, k) for b, k in zip(K.field_weights(kind), (1, 2))]
    for o in F.ORDERS:
        eh, es, er = F.emulate_field(dws, rws, K.field_feats()[rows], K.field_dirs()[rows], o)
        print("field %-8s order %-6s equal to the emulation: h %.4f  sigma %.4f  rgb %.4f" % (
            kind, o, same_value_share(h[rows], eh), float((sig[rows] == es).mean()), float((rgb[rows] == er).mean())))
        if PIN_EMULATED == o:
            assert same_value_share(h[rows], eh) == 1.0


def test_sigma_at_the_edges_of_h0(lib):
    c = K.sigma_edge_case()
    dw, rw = up(c.density_w), up(c.rgb_w)
    h, sig, rgb = run_field(lib, up(K.level_major(c.feats)), up(c.dirs), dw, rw, c.n)
    for res in K.check_field("trained", np.arange(c.n), h, sig, rgb, "sigma edges", dirs=c.dirs, ref=c.ref, rgb_w=c.rgb_w):
        ok(res)
    h0 = h[:, 0].astype(np.float64)
    assert np.array_equal(h0, c.feats[:, 0].astype(np.float64))
    assert np.isposinf(sig[h0 >= 89]).all() and (sig[h0 <= -104] == 0).all() and np.isfinite(sig[h0 <= 88.6875]).all()
    sub = (h0 > -104) & (h0 < -87.34)
    print("\nsigma for h0 in (-104, -87.34): %d samples, %d flushed to zero, %d subnormal" % (int(sub.sum()), int((sig[sub] == 0).sum()), int((sig[sub] != 0).sum())))
    # without h the same sigma, held against the h interval
    h2, sig2, rgb2 = run_field(lib, up(K.level_major(c.feats)), up(c.dirs), dw, rw, c.n, with_h=False)
    equal_bits(sig2, sig, "sigma without h_out")
    ok(F.check_sigma(sig2, c.ref.lo[:, 0], c.ref.hi[:, 0], what="sigma edges without h"))


def run_density(lib, feats, dw, n, with_h=True):
    h, sig = (buf16(n * 16) if with_h else None), buf32(n)
    lib.call("ngp_density_fwd", lib.ptr(feats), lib.ptr(dw), n, lib.ptr(sig), lib.ptr(h), lib.stream())
    torch.cuda.synchronize()
    return (take(h, n, 16) if with_h else None), take(sig, n, 1)[:, 0]


@pytest.mark.parametrize("n", (129, 65537, 2 * 65536 + 33))
def test_variants_of_one_computation_agree_bit_for_bit(lib, n):
    kind = "trained"
    dw, rw = field_dev(kind)
    feats, dirs = feats_dev(n), dirs_dev()
    h, sig, rgb = run_field(lib, feats, dirs, dw, rw, n)
    ref = K.density_reference(kind)
    # without h_out
    _, sig2, rgb2 = run_field(lib, feats, dirs, dw, rw, n, with_h=False)
    equal_bits(sig2, sig, "sigma without h_out")
    equal_bits(rgb2, rgb, "rgb without h_out")
    ok(F.check_sigma(sig2, ref.lo[:n, 0], ref.hi[:n, 0], what="sigma against the h interval"))
    # the density net alone
    hd, sigd = run_density(lib, feats, dw, n)
    equal_bits(hd, h, "h of ngp_density_fwd")
    equal_bits(sigd, sig, "sigma of ngp_density_fwd")
    _, sigd2 = run_density(lib, feats, dw, n, with_h=False)
    equal_bits(sigd2, sig, "sigma of ngp_density_fwd without h_out")
    # a device count below the launch bound: the count is also the level stride of the features
    for bound in (n, n + 1, n + 4 * F.SWEEP + 5):
        hb, sigb, rgbb = run_field(lib, feats, dirs, dw, rw, n, count=n, bound=bound)
        for got, full, cols in ((hb, h, 16), (sigb[:, None], sig[:, None], 1), (rgbb, rgb, 3)):
            equal_bits(np.ascontiguousarray(got[:n]), np.ascontiguousarray(full), "ngp_field_fwd_n bound %d" % bound)
            pre = PREFILL16 if got.dtype == np.float16 else PREFILL32
            assert (np.ascontiguousarray(got[n:]).view(np.int16 if got.dtype == np.float16 else np.int32) == pre).all(), "rows behind the count written"
    hb, sigb, rgbb = run_field(lib, feats, dirs, dw, rw, n, count=n + 77, bound=n)      # a count above the bound: the bound holds
    equal_bits(hb, h, "ngp_field_fwd_n count above the bound")
    equal_bits(rgbb, rgb, "ngp_field_fwd_n count above the bound")


def test_field_over_a_sample_list(lib):
    """More than 65 536 entries over 2 x 65 536 + 33 samples: -1 padding, ids >= stride, a padded entry as the last one of the first
    sweep and as the last one before the device count, a device count inside the list.  Listed samples equal the full launch bit for
    bit; all others keep the prefill."""
    kind, n = "trained", K.N_MAX
    dw, rw = field_dev(kind)
    feats, dirs = feats_dev(n), dirs_dev()
    h, sig, rgb = run_field(lib, feats, dirs, dw, rw, n)
    rng = np.random.RandomState(5)
    ids = rng.permutation(n)[:F.SWEEP + 3000].astype(np.int32)
    ids[::7] = -1
    ids[3::50] = n + rng.randint(0, 5, size=ids[3::50].shape)
    ids[5] = 2 ** 31 - 1
    ids[F.SWEEP - 1] = -1                                                          # a padded entry last in the first sweep
    for count in (None, F.SWEEP + 130, F.SWEEP + 2, 33):
        m = ids.size if count is None else count
        head = ids[:m].copy()
        if count is not None:
            head[m - 1] = -1                                                       # ... and last before the device count
        lst = np.concatenate([head, ids[m:][::-1]]) if count is not None else head  # entries behind the count are not read
        listed = head[(head >= 0) & (head < n)]
        assert count is None or m < ids.size
        hl, sigl, rgbl = run_field(lib, feats, dirs, dw, rw, n, lst=up(lst), n_list_max=ids.size, count=count, rows=n)
        rest = np.ones(n, bool)
        rest[listed] = False
        for got, full in ((hl, h), (sigl[:, None], sig[:, None]), (rgbl, rgb)):
            equal_bits(np.ascontiguousarray(got[listed]), np.ascontiguousarray(full[listed]), "list, count %s" % count)
            it = np.int16 if got.dtype == np.float16 else np.int32
            assert (np.ascontiguousarray(got[rest]).view(it) == (PREFILL16 if it == np.int16 else PREFILL32)).all(), "samples that are not listed were written"
        assert listed.size > (20 if count == 33 else 40000)


def test_density_scatter_keeps_the_largest(lib):
    """ngp_density_fwd_scatter into a zero-filled destination with repeated targets: sample s goes to cell s % 5003, so every cell has
    sources in different sweeps.  Each cell holds the maximum of its sources' sigmas bit for bit, on two runs; cells without a source
    and the guard stay zero."""
    kind, n, cells = "trained", K.N_MAX, 6000
    dw, _ = field_dev(kind)
    feats = feats_dev(n)
    _, sig = run_density(lib, feats, dw, n, with_h=False)
    ref = K.density_reference(kind)
    ok(F.check_sigma(sig, ref.lo[:n, 0], ref.hi[:n, 0], what="sigma of ngp_density_fwd without h"))
    idx = (np.arange(n) % 5003).astype(np.int32)
    assert (np.arange(n)[idx == 5002] // F.SWEEP).max() > (np.arange(n)[idx == 5002] // F.SWEEP).min()
    want = np.zeros(cells, np.float32)
    np.maximum.at(want, idx, sig)
    idx_d = up(idx)
    for run in range(2):
        out = torch.zeros(cells + GUARD, dtype=torch.float32, device="cuda")
        lib.call("ngp_density_fwd_scatter", lib.ptr(feats), lib.ptr(dw), n, lib.ptr(idx_d), lib.ptr(out), lib.stream())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        equal_bits(got[:cells], want, "scatter, run %d" % run)
        assert (got[5003:] == 0).all()
