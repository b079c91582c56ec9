"""TEST INFRASTRUCTURE -- weights, inputs, gradients, lists and counts for tests/test_field_backward_reference_cpu.py and
tests/test_field_backward_exact_gpu.py (the reference is tests/field_backward_reference.py).  Everything is numpy, seeded and cached
per process; it builds on tests/field_forward_cases.py (weights "trained" and "spread", inputs, field_feats, field_dirs).

A CASE is one launch: what goes in (by sample id or by compact position, as the contract says), the list, and `ref`, the intervals
of tests/field_backward_reference.py for the listed samples in compact order.  check_outputs() is THE check of a launch's outputs, shared
by the GPU tests and the CPU mutation tests."""
from types import SimpleNamespace

import numpy as np

from tests import field_backward_reference as B
from tests import field_forward_cases as FK
from tests import field_forward_reference as F

cached = FK.cached
CONFIGS, N_OUTS, WEIGHT_KINDS = FK.CONFIGS, FK.N_OUTS, FK.WEIGHT_KINDS
LOSS_SCALE = 128.0
LISTS = ("identity", "subset", "reversed", "count0", "count1", "count33", "countn", "over")
LIST_PAD = 64


def small_counts(w):
    return (1, 31, 32, 33, 32 * w - 1, 32 * w, 32 * w + 1)


def exact_counts(w):
    s = B.sweep(w)
    return small_counts(w) + (s - 1, s, s + 1, 2 * s + 33)


def ws_of(n_in, n_hidden, kind):
    return F.split_weights(FK.weights(n_in, n_hidden, kind), n_in, n_hidden)


# ---- gradients ------------------------------------------------------------------------------------------------------------------------
@cached
def dout(n, tag=0):
    """dL_dout (n, 16) f16, about 0.1 N(0, 1), every fifth row zero."""
    d = (np.random.RandomState(700 + tag).randn(n, 16) * 0.1).astype(np.float16)
    d[::5] = 0
    return d


@cached
def seeds(n):
    """dL_dsigmas (n,) about 1e-3 N(0, 1) and dL_drgbs (n, 3) about 1e-2 N(0, 1), f32, every fifth sample zero."""
    rng = np.random.RandomState(701)
    s, c = (rng.randn(n) * 1e-3).astype(np.float32), (rng.randn(n, 3) * 1e-2).astype(np.float32)
    s[::5], c[::5] = 0, 0
    return s, c


# ---- lists ----------------------------------------------------------------------------------------------------------------------------
@cached
def make_list(name, n):
    """(buffer int32, *n_active).  The buffer is longer than *n_active wherever that fits, with -1 and ids >= n behind it."""
    rng = np.random.RandomState(800 + n)
    tail = np.where(np.arange(LIST_PAD) % 2 == 0, -1, n + np.arange(LIST_PAD)).astype(np.int32)
    perm = rng.permutation(n).astype(np.int32)
    if name == "identity":
        head, count = np.arange(n, dtype=np.int32), n
    elif name == "subset":
        head = np.sort(perm[:max(1, (3 * n) // 5)])
        count = head.size
    elif name == "reversed":
        head, count = np.arange(n, dtype=np.int32)[::-1].copy(), n
    elif name == "countn":
        head, count = perm, n
    elif name == "over":
        head, count = perm, n + 1000
        tail = np.resize(tail, 1000 + LIST_PAD)
    else:
        count = int(name[5:])
        assert name.startswith("count") and count <= n
        head = perm[:count]
    return np.concatenate([head, tail]).astype(np.int32), count


def resolve(lst, n):
    """active buffer, *n_active, n_eff, ids (n_eff,) of a list name (None: no list)."""
    if lst is None:
        return None, None, n, np.arange(n)
    buf, count = make_list(lst, n)
    n_eff = min(count, n)
    return buf, count, n_eff, buf[:n_eff].astype(np.int64)


# ---- ngp_mlp_bwd ----------------------------------------------------------------------------------------------------------------------
@cached
def plain_case(n_in, n_hidden, kind, n, n_out, act):
    ws, w = ws_of(n_in, n_hidden, kind), B.waves(n_in, n_hidden)
    x, d = FK.inputs(n_in)[:n], np.ascontiguousarray(dout(n, n_in)[:, :n_out])
    counts = [c for c in small_counts(w) if c <= n] + [n]
    ref = B.mlp_backward_intervals(ws, x, None, B.plain_dy(d, n_out, act), w, counts)
    return SimpleNamespace(family="plain", ws=ws, blob=FK.weights(n_in, n_hidden, kind), inputs=x, dout=d, n_out=n_out, out_act=act, seed=None,
                           scale=1.0, active=None, n_active=None, n_samples=n, n_eff=n, w=w, ref=ref, dirs=None,
                           what="mlp %d-%d %s n_out=%d act=%d" % (n_in, n_hidden, kind, n_out, act), n_in=n_in, n_hidden=n_hidden)


def prefix(case, n):
    """The launch over the first n samples of a case without a list (its dW intervals come from the one cumulative pass)."""
    assert case.active is None and n in case.ref.dw
    c = SimpleNamespace(**vars(case))
    c.n_samples = c.n_eff = n
    c.inputs = case.inputs[:n]
    c.dout = None if case.dout is None else case.dout[:n]
    c.seed = None if case.seed is None else case.seed[:n]
    c.dirs = None if case.dirs is None else case.dirs[:n]
    c.what = "%s n=%d" % (case.what, n)
    return c


@cached
def exact_case(n_in, n_hidden):
    """The exact net over 2 sweeps + 33 samples: dL_dout non-zero on the first 32 W + 64 rows (all small counts are dense), on the first
    and last 64 rows of each sweep and on the last 33 rows.  Returns blob, x, dout, {n_out: (din, dw[count])}."""
    w = B.waves(n_in, n_hidden)
    s = B.sweep(w)
    n = 2 * s + 33
    rows = [np.arange(32 * w + 64), np.arange(n - 33, n)]
    for k in range(3):
        rows += [np.arange(k * s, min(k * s + 64, n)), np.arange(max(0, (k + 1) * s - 64), min((k + 1) * s, n))]
    blob, x, d = B.exact_backward_net(n_in, n_hidden, n, seed=n_in + n_hidden, nonzero_rows=np.concatenate(rows))
    ws = F.split_weights(blob, n_in, n_hidden)
    want = {n_out: B.backward_point(ws, x, B.pad16(d, n_out), exact_counts(w)) for n_out in N_OUTS}
    return SimpleNamespace(blob=blob, x=x, dout=d, want=want, w=w, n=n, ws=ws)


# ---- the density net ------------------------------------------------------------------------------------------------------------------
CLAMP_H0 = (0.0, 14.99, -14.99, 15.0, -15.0, 15.01, -15.01, 20.0, -20.0)


@cached
def density_weights(name):
    """blob and row-major features (N, 32).  trained / spread: the field's.  clamp: the sigma_edge_case construction (h0 = x0 exactly)
    with h0 around the clamp of the TruncExp backward.  underflow: |w|, |x| in [0.5, 1) * 2^-11, all normal f16 values, so that the
    pre-activations are sums of 32 products of about 2^-23: positive ones below 2^-25 are stored as f16 zero."""
    n = 4096
    if name in WEIGHT_KINDS:
        return FK.field_weights(name)[0], FK.field_feats()
    if name == "clamp":
        W0, Wo = [m.copy() for m in F.split_weights(FK.field_weights("trained")[0], 32, 1)]
        W0[0], W0[1], Wo[0] = 0, 0, 0
        W0[0, 0], W0[1, 0], Wo[0, 0], Wo[0, 1] = 1, -1, 1, -1
        feats = FK.field_feats()[:n].copy()
        feats[:, 0] = np.resize(np.array(CLAMP_H0, np.float16), n)
        return np.concatenate([W0.reshape(-1), Wo.reshape(-1)]), feats
    assert name == "underflow"
    rng = np.random.RandomState(811)
    mag = lambda *shape: rng.choice([-1.0, 1.0], size=shape) * rng.uniform(0.5, 1.0, size=shape) * 2.0 ** -11
    W0, feats = mag(F.HID, 32).astype(np.float16), mag(n, 32).astype(np.float16)
    assert (np.abs(W0) >= 2.0 ** -14).all() and (np.abs(feats) >= 2.0 ** -14).all()
    pre = feats.astype(np.float64) @ W0.astype(np.float64).T
    assert ((pre > 0) & (F.f16(pre) == 0)).sum() > 1000, "no positive pre-activation underflows"
    Wo = F.split_weights(FK.field_weights("trained")[0], 32, 1)[1] * np.float16(2.0 ** 10)
    return np.concatenate([W0.reshape(-1), Wo.reshape(-1)]), feats


@cached
def density_case(name, n, lst=None, with_dh=True, with_sigma=True):
    blob, feats = density_weights(name)
    ws = F.split_weights(blob, 32, 1)
    assert n <= feats.shape[0]
    active, n_active, n_eff, ids = resolve(lst, n)
    dh = dout(n, 99) if with_dh else None
    sig = seeds(n)[0] if with_sigma else None
    if name == "clamp" and sig is not None:
        sig = sig * np.float32(2.0 ** -8)               # exp(15) = 3.3e6: keeps seed * 128 * exp(h0) inside the f16 range
    counts = ([c for c in small_counts(8) if c <= n_eff] + [n_eff]) if lst is None else [n_eff]
    ref = None
    if n_eff:
        ref = B.density_backward_intervals(ws, feats[ids], None if dh is None else dh[:n_eff], None, None if sig is None else sig[ids],
                                           B.scale32(LOSS_SCALE), 8, counts)
    return SimpleNamespace(family="density", ws=ws, blob=blob, inputs=feats[:n], dout=dh, n_out=16, out_act=0, seed=sig, scale=B.scale32(LOSS_SCALE),
                           active=active, n_active=n_active, n_samples=n, n_eff=n_eff, w=8, ref=ref, dirs=None,
                           what="density %s n=%d list=%s dh=%d sigma=%d" % (name, n, lst, with_dh, with_sigma))


@cached
def exact_density_case(n=257):
    """The exact 32-64-16 net with row 0 of Wo zeroed: h0 = 0 for every sample, __expf(0) = 1, and with seeds k * 2^-11 (times the
    loss scale 128: k * 2^-4) the TruncExp path is exact too.  Returns the case and the expected din (n, 32) and dW."""
    blob, x, d = B.exact_backward_net(32, 1, n, seed=77)
    ws = [m.copy() for m in F.split_weights(blob, 32, 1)]
    ws[1][0] = 0
    blob = np.concatenate([m.reshape(-1) for m in ws])
    sig = (np.random.RandomState(78).randint(-2, 3, size=n) * 2.0 ** -11).astype(np.float32)
    dy = B.density_point_dy(d, sig, B.scale32(LOSS_SCALE))
    want = B.backward_point(ws, x, dy, small_counts(8))
    g = dy(np.zeros((n, 16))).astype(np.float64)
    assert np.array_equal(g[:, 0], d[:, 0].astype(np.float64) + sig.astype(np.float64) * 128.0)
    B.assert_backward_exact(ws, x, g, 2.0 ** -4)
    case = SimpleNamespace(family="density", ws=ws, blob=blob, inputs=x, dout=d, n_out=16, out_act=0, seed=sig, scale=B.scale32(LOSS_SCALE),
                           active=None, n_active=None, n_samples=n, n_eff=n, w=8, ref=None, dirs=None, what="exact density")
    return case, want


# ---- the field ------------------------------------------------------------------------------------------------------------------------
@cached
def field_case(kind, n, lst=None, dev_scale=None):
    """field_bwd_kernel: ref = (density intervals, colour intervals), everything propagated from the features."""
    dw, rw = FK.field_weights(kind)
    dws, rws = F.split_weights(dw, 32, 1), F.split_weights(rw, 32, 2)
    active, n_active, n_eff, ids = resolve(lst, n)
    feats, dirs = FK.field_feats()[:n], FK.field_dirs()[:n]
    sig, rgb = seeds(n)
    scale = B.scale32(LOSS_SCALE, dev_scale)
    counts = ([c for c in small_counts(4) if c <= n_eff] + [n_eff]) if lst is None else [n_eff]
    ref = B.field_backward_intervals(dws, rws, feats[ids], dirs[ids], sig[ids], rgb[ids], scale, counts) if n_eff else None
    return SimpleNamespace(family="field", dws=dws, rws=rws, dw=dw, rw=rw, feats=feats, dirs=dirs, sig=sig, rgb=rgb, scale=scale, dev_scale=dev_scale,
                           active=active, n_active=n_active, n_samples=n, n_eff=n_eff, ids=ids, ref=ref, w=4,
                           what="field %s n=%d list=%s dev=%s" % (kind, n, lst, dev_scale))


def field_prefix(case, n):
    assert case.active is None and n in case.ref[0].dw
    c = SimpleNamespace(**vars(case))
    c.n_samples = c.n_eff = n
    c.feats, c.dirs, c.sig, c.rgb, c.ids = case.feats[:n], case.dirs[:n], case.sig[:n], case.rgb[:n], case.ids[:n]
    c.what = "%s prefix %d" % (case.what, n)
    return c


@cached
def arbitrary_h(n):
    """An f16 h (n, 16) that is NOT the density net's: ngp_field_bwd_two_launches takes h as an input."""
    return (np.random.RandomState(702).randn(n, 16) * 0.7).astype(np.float16)


# ---- the check ------------------------------------------------------------------------------------------------------------------------
def rows_of(din_buf, family):
    """The din buffer of a launch as (n_samples, columns) by compact position."""
    return np.ascontiguousarray(din_buf.transpose(1, 0, 2)).reshape(din_buf.shape[1], 32) if family in ("density", "field") else din_buf


def untouched(a):
    """Every value still carries the NaN prefill."""
    a = np.ascontiguousarray(a)
    return bool((a.view(np.uint16) == 0x7E5A).all()) if a.dtype == np.float16 else bool((a.view(np.uint32) == 0x7FC5A5A5).all())


def check_outputs(ref, n_eff, din_rows, part, what):
    """din (by compact position) and the float64 sum of ALL partial rows against the intervals; positions >= n_eff must carry the
    prefill (counted as outside otherwise).  n_eff == 0: every partial row exactly zero.  Returns the F.check results."""
    part64 = np.asarray(part, np.float64).sum(axis=0)
    if n_eff == 0:
        z = np.zeros_like(part64)
        res = [F.check(np.abs(np.asarray(part, np.float64)).sum(axis=0), z, z, what + " dW of an empty launch")]
    else:
        res = [F.check(din_rows[:n_eff], ref.din_lo[:n_eff], ref.din_hi[:n_eff], what + " din"), F.check(part64, *ref.dw[n_eff], what=what + " dW")]
    if not untouched(din_rows[n_eff:]):
        res.append(SimpleNamespace(bad=1, n=1, worst=what + ": positions >= n_eff were written"))
    return res


def emulate_case(case, mut=None):
    """The CPU emulation of the case's launch -> the F.check results of check_outputs (the field: density and colour)."""
    if case.family == "field":
        dfeats, part_d, part_r, dh, h = B.emulate_field_backward(case.dws, case.rws, case.feats, case.dirs, case.sig, case.rgb, case.scale,
                                                                case.n_samples, case.active, case.n_active, mut)
        return check_field_outputs(case, dfeats, part_d, part_r, h, dh)
    din, part = B.emulate_backward(case.family, case.ws, case.inputs, case.n_samples, case.w, case.dout, case.n_out, case.out_act, case.seed,
                                   case.scale, case.active, case.n_active, case.dirs, mut)
    return check_outputs(case.ref, case.n_eff, rows_of(din, case.family), part, case.what)


def check_field_outputs(case, dfeats, part_d, part_r, h=None, dh=None, pin_c=None):
    """One launch of field_bwd_kernel.  dfeats and both dW blobs against the intervals propagated from the FEATURES (wide: eight
    layers of interval arithmetic), and -- THE sharp check of its dW -- against intervals from PINNED hand-overs: h (n_samples, 16) by
    sample id, the forward's own, pins the colour net's input, and dh (>= n_eff, 16) by compact position, the dL/dh of the two-launch
    chain fed that h, pins the density net's output gradient (the caller has shown dfeats bit-equal to that chain's)."""
    ref_d, ref_c = case.ref if case.ref is not None else (None, None)
    res = check_outputs(ref_d, case.n_eff, rows_of(dfeats, "field"), part_d, case.what + " density net")
    part64 = np.asarray(part_r, np.float64).sum(axis=0)
    if case.n_eff:
        res.append(F.check(part64, *ref_c.dw[case.n_eff], what=case.what + " colour net dW"))
    else:
        res.append(F.check(np.abs(np.asarray(part_r, np.float64)).sum(axis=0), np.zeros_like(part64), np.zeros_like(part64), case.what + " colour dW, empty"))
    if h is not None and case.n_eff:
        n_eff, ids = case.n_eff, case.ids
        if pin_c is None:                                               # (a caller may have it already: it is the two-launch chain's)
            pin_c = B.colour_backward_intervals(case.rws, case.dirs[ids], h[ids], None, case.rgb[ids], case.scale, [n_eff])
        pin_d = B.density_backward_intervals(case.dws, case.feats[ids], dh[:n_eff], None, case.sig[ids], case.scale, 4, [n_eff])
        res.append(F.check(part64, *pin_c.dw[n_eff], what=case.what + " colour net dW from the pinned h"))
        res.append(F.check(np.asarray(part_d, np.float64).sum(axis=0), *pin_d.dw[n_eff], what=case.what + " density net dW from the pinned dL/dh"))
        res.append(F.check(rows_of(dfeats, "field")[:n_eff], pin_d.din_lo, pin_d.din_hi, case.what + " dfeats from the pinned dL/dh"))
    return res
