"""TEST INFRASTRUCTURE -- weights, inputs and counts for tests/test_field_forward_reference_cpu.py and tests/test_field_forward_exact_gpu.py
(the reference is tests/field_forward_reference.py).  Everything is numpy, seeded, and cached per process: a reference is computed once
for the largest count and shared; every smaller count is a prefix of it (samples are independent)."""
import math
from types import SimpleNamespace

import numpy as np

from tests import field_forward_reference as F

# around the 32-sample tile, the 128-sample workgroup and the 65 536-sample sweep of the capped launch; the last one gives some waves a
# third tile (and the list variant its second prefetch)
COUNTS = (1, 31, 32, 33, 127, 128, 129, 65535, 65536, 65537, 65536 + 129, 2 * 65536 + 33)
N_MAX = COUNTS[-1]
CONFIGS = tuple((n_in, n_hidden) for n_in in (16, 32, 64) for n_hidden in (1, 2))
N_OUTS = (1, 3, 8, 16)
WEIGHT_KINDS = ("trained", "spread")
_CACHE = {}


def cached(fn):
    def wrapper(*args):
        key = (fn.__name__,) + args
        if key not in _CACHE:
            _CACHE[key] = fn(*args)
        return _CACHE[key]
    wrapper.__name__ = fn.__name__
    return wrapper


def _xavier(rng, o, i):
    a = math.sqrt(6.0 / (i + o))
    return (rng.rand(o, i) * 2 - 1) * a


@cached
def weights(n_in, n_hidden, kind, seed=0):
    """The tight f16 blob.  trained: xavier-uniform x 1.5, the magnitudes of the `field` fixture of tests/test_field_gpu.py.  spread: the
    same with every entry scaled by its own power of two from 2^-9 to 2^2, so small weights sit next to large ones."""
    rng = np.random.RandomState(1000 * n_in + 10 * n_hidden + seed + (7 if kind == "spread" else 0))
    dims = [n_in] + [F.HID] * n_hidden + [16]
    ws = [_xavier(rng, dims[i + 1], dims[i]) * 1.5 for i in range(len(dims) - 1)]
    if kind == "spread":
        ws = [w * 2.0 ** rng.randint(-9, 3, size=w.shape) for w in ws]
    else:
        assert kind == "trained"
    return np.concatenate([w.reshape(-1) for w in ws]).astype(np.float16)


@cached
def inputs(n_in, n=N_MAX):
    """N(0, 1) f16 row-major inputs for ngp_mlp_fwd."""
    return np.random.RandomState(50 + n_in).randn(n, n_in).astype(np.float16)


@cached
def mlp_reference(n_in, n_hidden, kind):
    return F.mlp_intervals(F.split_weights(weights(n_in, n_hidden, kind), n_in, n_hidden), inputs(n_in))


def emulation_rows(n):
    """The rows of a launch of n samples that the (slow) emulation is run on: its head and its tail."""
    return np.arange(n) if n <= 4096 else np.concatenate([np.arange(2048), np.arange(n - 2048, n)])


# ---- nets in which every output is ONE product ----------------------------------------------------------------------------------------
ONE_HOT_VALUES = (1.0, -0.7197265625, 3.140625, -0.0011997222900390625)       # f16 values: plain, 10-bit, large, small


def _selection_first(n_in, shift):
    """W0 (64, n_in) with W0[(k + shift) % 64, k] = 1: input unit k lands on hidden unit (k + shift) % 64."""
    W = np.zeros((F.HID, n_in))
    W[(np.arange(n_in) + shift) % F.HID, np.arange(n_in)] = 1
    return W


def _selection_out(block):
    W = np.zeros((16, F.HID))
    W[np.arange(16), 16 * block + np.arange(16)] = 1
    return W


def one_hot_cases(n_in, n_hidden):
    """Yields (name, blob, x, expected (n, 16) f16): dense random weights in ONE matrix, 0 / 1 selections in the others, one-hot inputs
    +-v e_k.  Every output is then relu(f16(w_jk v)) (the output layer: f16(w_jk v)), and every (j, k) of every matrix is covered."""
    rng = np.random.RandomState(77 + n_in + n_hidden)
    x = np.zeros((n_in * len(ONE_HOT_VALUES) * 2, n_in))
    r = 0
    for k in range(n_in):
        for v in ONE_HOT_VALUES:
            for sign in (1, -1):
                x[r, k] = sign * v
                r += 1
    assert np.array_equal(x.astype(np.float16).astype(np.float64), x), "one-hot values must be f16 values"
    x = x.astype(np.float16)
    dense = lambda o, i: (_xavier(rng, o, i) * 1.5).astype(np.float16).astype(np.float64)
    eye = np.eye(F.HID)
    nets = []
    for block in range(4):                                              # W0 dense: the output layer shows 16 hidden units at a time
        nets.append(("W0 block %d" % block, [dense(F.HID, n_in)] + [eye] * (n_hidden - 1) + [_selection_out(block)]))
    for shift in range(0, F.HID, n_in):                                 # the input reaches hidden units shift .. shift + n_in - 1
        if n_hidden == 2:
            for block in range(4):
                nets.append(("W1 shift %d block %d" % (shift, block), [_selection_first(n_in, shift), dense(F.HID, F.HID), _selection_out(block)]))
        nets.append(("Wo shift %d" % shift, [_selection_first(n_in, shift)] + [eye] * (n_hidden - 1) + [dense(16, F.HID)]))
    for name, ws in nets:
        ws16 = [w.astype(np.float16) for w in ws]
        a = x.astype(np.float64)
        for i, w in enumerate(ws):                                      # at most one non-zero product per sum: float64 is exact here
            assert ((a[:, None, :] * w[None]) != 0).sum(axis=2).max() <= 1
            a = F.f16(a @ w.T).astype(np.float64)
            if i < len(ws) - 1:
                a = np.maximum(a, 0) + 0.0                               # ReLU gives +0, also for the -0 of a tiny negative product
        yield name, np.concatenate([w.reshape(-1) for w in ws16]), x, F.f16(a)


def passthrough_case(n_in, n_hidden, block, n=4099):
    """A dense trained-like W0 on dense N(0, 1) inputs, identity / selection behind it: the output is relu(f16(accumulator)) of ONE
    layer from pinned inputs, for hidden units 16 block .. 16 block + 15.  Returns blob, x, s, e (n, 16) of those units."""
    ws = F.split_weights(weights(n_in, n_hidden, "trained"), n_in, n_hidden)
    W0 = ws[0]
    mats = [W0] + [np.eye(F.HID).astype(np.float16)] * (n_hidden - 1) + [_selection_out(block).astype(np.float16)]
    x = inputs(n_in)[:n]
    s, _, e = F.layer_interval(W0, x.astype(np.float64), x.astype(np.float64))
    return np.concatenate([m.reshape(-1) for m in mats]), x, s[:, 16 * block:16 * block + 16], e[:, 16 * block:16 * block + 16]


# ---- the field ------------------------------------------------------------------------------------------------------------------------
FIELD_KINDS = WEIGHT_KINDS


@cached
def field_weights(kind):
    return weights(32, 1, kind, 3), weights(32, 2, kind, 4)


@cached
def field_feats(n=N_MAX):
    """Row-major (n, 32) f16 features, uniform in [-0.8, 0.8] like a trained table's."""
    return ((np.random.RandomState(60).rand(n, 32) * 2 - 1) * 0.8).astype(np.float16)


def level_major(feats_rm):
    """(n, 32) row-major -> [16][n][2], the layout the field kernels read."""
    n = feats_rm.shape[0]
    return np.ascontiguousarray(feats_rm.reshape(n, 16, 2).transpose(1, 0, 2))


@cached
def field_dirs(n=N_MAX):
    """Un-normalised f32 directions with norms from 1e-3 to 1e3; the first rows are the axes and the poles at several norms."""
    rng = np.random.RandomState(61)
    d = rng.randn(n, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d *= 10.0 ** rng.uniform(-3, 3, size=(n, 1))
    special = []
    for norm in (1.0, 1e-3, 1e3, 0.37):
        for axis in range(3):
            for sign in (1.0, -1.0):
                v = [0.0, 0.0, 0.0]
                v[axis] = sign * norm
                special.append(v)
    special += [[1.0, 1.0, 0.0], [0.0, -2.0, 2.0], [3.0, 0.0, 3.0], [1e-3, 1e-3, 1e3], [5.0, 5.0, 5.0]]
    special = np.array(special)
    m = min(n, special.shape[0])
    d[:m] = special[:m]
    return d.astype(np.float32)


@cached
def density_reference(kind):
    """The h interval of every row of field_feats() (lo / hi (n, 16) f16)."""
    dw, _ = field_weights(kind)
    return F.mlp_intervals(F.split_weights(dw, 32, 1), field_feats())


# h[0] edges: hidden unit 0 = relu(x0), hidden unit 1 = relu(-x0), h0 = hidden 0 - hidden 1 = x0 exactly; every other row of both
# matrices is the trained-like one, so h[1:] and rgb stay ordinary.
SIGMA_EDGE_H0 = (11.0, -11.0, 88.0, 88.5, 88.6875, 88.75, 89.0, 89.0625, 100.0, 1000.0, -80.0, -87.0, -87.3125, -87.375, -88.0, -90.0, -95.0,
                 -100.0, -103.0, -103.9375, -104.0, -104.0625, -110.0, -1000.0, 0.0, -0.0)


@cached
def sigma_edge_case(n=4096 + 33):
    dw, rw = field_weights("trained")
    W0, Wo = [w.copy() for w in F.split_weights(dw, 32, 1)]
    W0[0], W0[1] = 0, 0
    W0[0, 0], W0[1, 0] = 1, -1
    Wo[0] = 0
    Wo[0, 0], Wo[0, 1] = 1, -1
    feats = field_feats(n).copy()
    h0 = np.array(SIGMA_EDGE_H0, np.float16)
    assert np.array_equal(h0.astype(np.float64), np.array(SIGMA_EDGE_H0))
    feats[:, 0] = np.resize(h0, n)
    blob = np.concatenate([W0.reshape(-1), Wo.reshape(-1)])
    ref = F.mlp_intervals([W0, Wo], feats)
    assert np.array_equal(ref.lo[:, 0], ref.hi[:, 0]) and np.array_equal(ref.lo[:, 0].astype(np.float64), np.abs(feats[:, 0].astype(np.float64)) * np.sign(feats[:, 0].astype(np.float64)))
    return SimpleNamespace(density_w=blob, rgb_w=rw, feats=feats, dirs=field_dirs(n), ref=ref, n=n)


def check_field(kind, rows, h, sigma, rgb, what, dirs=None, ref=None, rgb_w=None):
    """The three checks of one field launch, on the samples `rows` of the committed case: h inside the interval from the features, sigma
    against the launch's OWN h[0], rgb inside the interval propagated from the launch's OWN h (and an f16 value).  Returns the three
    results of F.check."""
    ref = density_reference(kind) if ref is None else ref
    rgb_w = field_weights(kind)[1] if rgb_w is None else rgb_w
    dirs = field_dirs()[rows] if dirs is None else dirs
    rh = F.check(h, ref.lo[rows], ref.hi[rows], what + " h")
    rs = F.check_sigma(sigma, h[:, 0], what=what + " sigma")
    pinned = np.where(np.isfinite(h.astype(np.float32)), h, np.float16(0))          # an unwritten h has failed above already
    lo, hi = F.colour_intervals(F.split_weights(rgb_w, 32, 2), dirs, pinned)
    rr = F.check_rgb(rgb, lo, hi, what + " rgb")
    return rh, rs, rr
