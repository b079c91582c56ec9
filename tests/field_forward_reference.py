"""TEST INFRASTRUCTURE -- the forward of the fused MLPs of csrc/mlp.hip (ngp_mlp_fwd, ngp_density_fwd, ngp_field_fwd and its variants)
restated in numpy float64 from their CONTRACT: f16 inputs and weights (out, in) row-major, no bias, ReLU on the hidden layers, f32
accumulation over the whole K, f16 activations between layers, output layer padded to 16 rows.  No waves, tiles or fragments in here.

ONE LAYER.  Inputs and weights are f16, so every product w_k a_k has at most 22 significant bits and is exact in f32.  With

    s = sum_k w_k a_k   and   mass = sum_k |w_k| |a_k|       in float64,

the MODEL of the kernel's f32 accumulator is: the K exact products are added in an order we do not know, and every addition is off by
at most 2^-23 relative to its result (that covers round to nearest, 2^-24, and truncation after alignment, 2^-23).  Every partial sum
is bounded by mass, there are at most K additions, hence

    accumulator in [s - e, s + e],   e = K * 2^-23 * mass.

THE 2^-23 IS AN ASSUMPTION: the numerics of v_mfma_f32_32x32x16_f16 (what it rounds, and where, inside its sixteen-term dot product)
are not published in the material this project has; only an f32-input MFMA is described there, as a k-ordered fmaf chain.  DESIGN.md
section 19 records how the first run on an MI355X put the assumption to the test.  The float64 evaluation of s and mass is itself off
by less than K * 2^-53 * mass, 2^-30 of e.

The conversion f32 -> f16 (round to nearest even) and ReLU are monotone, so the stored activation lies in

    [relu(f16(s - e)), relu(f16(s + e))]

and NO output has to be excluded: an interval around the exact pre-activation maps to an interval of f16 values.  A layer whose inputs
are intervals [lo, hi] gets  s_lo = W+ lo + W- hi,  s_hi = W+ hi + W- lo,  mass = |W| max(|lo|, |hi|)  (W+ / W- the positive / negative
parts of W), and e from that mass.

OUTPUTS.
  h      the f16 interval of the density net's output layer.
  sigma  the kernel computes __expf((float)h[0]) on its own f16 h[0].  Where h is written, sigma is held against exp of the KERNEL's
         h[0] in float64 within relative (|h0| + 3) * 2^-23: 2 ulp (2 * 2^-23) for the hardware exponential behind __expf, as
         tests/test_vren_gpu.py allows, and |h0| * 2^-24 * (1 + 1/2) < |h0| * 2^-23 for the one rounding of h0 * log2(e) and that of the
         constant (an error d of the exponent of 2 moves the result by ln2 * d relative); the remaining 2^-23 covers second-order terms.
         Where h is not written (h_out = NULL, ngp_density_fwd_scatter) sigma is held against exp of the h interval with the same slack.
         Range: at or above h0 = 89, exp(h0) > FLT_MAX and +inf is required; at or below -104, exp(h0) < 2^-150 and exactly 0 is
         required; where exp(h0) < 2^-126 (h0 < -87.33) a flushed 0 is accepted next to the subnormal within the limit plus one
         subnormal spacing (2^-149).
  rgb    the kernel computes (float)(half) (1 / (1 + __expf(-c))) from the f32 accumulator c of the output layer.  With t = exp(-c):
         __expf(-c) = t (1 + a), |a| <= (|c| + 3) 2^-23 as above; 1 + t(1 + a) = (1 + t)(1 + a t / (1 + t)), and t / (1 + t) < 1, so
         the sum is off by at most |a| relative, plus 2^-24 for its own rounding; the division adds 2^-23 (one ulp: correctly rounded
         or the hardware reciprocal).  Altogether sigmoid' = sigmoid(c) (1 + d), |d| <= DELTA(c) = ((|c| + 3) 2^-23 + 3 * 2^-24) * 1.001
         (the factor holds the second-order terms).  Sigmoid is monotone, so with c in [c_lo, c_hi]
             rgb in [f16(sigmoid(c_lo) (1 - DELTA(c_lo))), f16(sigmoid(c_hi) (1 + DELTA(c_hi)))]
         and rgb must be exactly representable in f16.  (Where t overflows or flushes, sigmoid' is 0 or 1 and so are the bounds.)
  colour net input.  Chunk 1 is the KERNEL's own h (exact values, width 0): the colour net is three layers from pinned inputs.  Chunk 0
         is SH(d / |d|): sh_interval() evaluates the sixteen polynomials in float64 with the kernel's f32 constants and bounds the f32
         evaluation by roundings counted, u = 2^-24 (sqrt and division taken as 2u each, in case they are not correctly rounded):
           |d|^2   three products (1 + u), each through at most two additions: 3u;  its square root 1.5u + 2u;  1 / that: + 2u;
           x = dx * inv: + u   ->  x, y, z carry at most 6.5u each.
           A coefficient is C * (a monomial sum of degree <= 3): 3 * 6.5u = 19.5u from the inputs, at most 6 roundings of its own
           operations (x2, 5 * z2, the sum, C * y, the product, one spare) -> 25.5u, rounded up to 32u = 2^-19 of
           mass = sum of the absolute values of its monomials (contraction is off in sh4(): the operations are the ones written).
         Then the f16 rounding is applied to both ends.

EXACT NETS (exact_net()).  Weights and inputs that are integer multiples of a power of two, with mass <= 2048 units in every layer:
every product, every partial sum in any order and every pre-activation is then representable in f16 (and f32), any summation order
gives the same bits, and the expected output needs no numerics model.  The generator asserts that condition.

EMULATION (emulate_mlp / emulate_field).  The kernel as a k-ordered chain per layer, acc = f32(acc + w_k a_k) from 0 (the product is
exact, so this is fmaf), K order selectable: "asc", "desc", or "kernel" (natural order for chunks that come from memory, the D order of
the header of csrc/mlp.hip, unit 16c + 4hh + (e & 3) + 8(e >> 2), for chunks that are a previous layer's fragment).  `mut` names a
deliberately wrong kernel (MUTANTS) for tests/test_field_forward_reference_cpu.py."""
from types import SimpleNamespace

import numpy as np

U23 = 2.0 ** -23
U24 = 2.0 ** -24
F32_MAX = float(np.finfo(np.float32).max)
F32_MIN_NORMAL = 2.0 ** -126
F32_MIN_SUB = 2.0 ** -149
HID = 64
TILE, SWEEP = 32, 65536          # samples per wave tile, and per sweep of the capped launch (512 workgroups x 4 waves x 32)


# ------------------------------------------------------------------------------------------------------------------ f16 helpers
def f16(x):
    """float64 -> f16, round to nearest even, overflow to inf (numpy converts double to half directly: one rounding)."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(np.float16)


def ord16(h):
    """f16 -> int32, monotone in the value, +0 and -0 both 0: the difference of two is their distance in f16 values."""
    b = np.ascontiguousarray(h, np.float16).view(np.int16).astype(np.int32)
    return np.where(b >= 0, b, -(b & 0x7FFF))


def is_f16_value(v):
    v = np.asarray(v)
    with np.errstate(over="ignore", invalid="ignore"):
        return v.astype(np.float16).astype(v.dtype) == v


def f16_trunc(a32):
    """f32 -> f16 toward zero (a wrong kernel's conversion)."""
    with np.errstate(over="ignore"):
        r = np.asarray(a32, np.float32).astype(np.float16)
    over = np.abs(r.astype(np.float64)) > np.abs(np.asarray(a32, np.float64))
    bits = r.view(np.uint16).copy()
    bits[over] -= 1
    return bits.view(np.float16)


def split_weights(blob, n_in, n_hidden):
    """The tight blob: W0 (64, n_in), W1 (64, 64) if n_hidden == 2, Wo (16, 64), each (out, in) row-major."""
    blob = np.asarray(blob)
    assert blob.dtype == np.float16 and blob.ndim == 1
    dims = [n_in] + [HID] * n_hidden + [16]
    ws, off = [], 0
    for i in range(len(dims) - 1):
        ws.append(blob[off:off + dims[i + 1] * dims[i]].reshape(dims[i + 1], dims[i]))
        off += dims[i + 1] * dims[i]
    assert off == blob.size, (off, blob.size)
    return ws


# ------------------------------------------------------------------------------------------------------------------ intervals
def layer_interval(W, lo, hi):
    """W (O, K) f16, inputs in [lo, hi] (n, K) float64 -> s_lo, s_hi, e (n, O): the f32 accumulator lies in [s_lo - e, s_hi + e]."""
    W = W.astype(np.float64)
    Wp, Wn = np.maximum(W, 0), np.minimum(W, 0)
    s_lo = lo @ Wp.T + hi @ Wn.T
    s_hi = s_lo if hi is lo else hi @ Wp.T + lo @ Wn.T
    mass = np.maximum(np.abs(lo), np.abs(hi)) @ np.abs(W).T
    e = W.shape[1] * U23 * mass
    if not (np.isfinite(s_lo).all() and np.isfinite(s_hi).all()):
        raise ValueError("a pre-activation that is not finite: outside what the intervals cover")
    return s_lo, s_hi, e


def activation_interval(s_lo, s_hi, e, relu):
    lo, hi = f16(s_lo - e), f16(s_hi + e)
    if relu:
        lo, hi = np.maximum(lo, np.float16(0)), np.maximum(hi, np.float16(0))
        if not np.isfinite(hi.astype(np.float64)).all():
            raise ValueError("a hidden activation beyond the f16 range: outside what the intervals cover")
    return lo, hi


def sigmoid(c):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(c, np.float64)))


def delta_sigmoid(c):
    return ((np.abs(c) + 3.0) * U23 + 3.0 * U24) * 1.001


def sigmoid_interval(c_lo, c_hi):
    """The f32 accumulator in [c_lo, c_hi] -> the f16 interval of (half)(1 / (1 + __expf(-c)))."""
    return f16(sigmoid(c_lo) * (1.0 - delta_sigmoid(c_lo))), f16(np.minimum(sigmoid(c_hi) * (1.0 + delta_sigmoid(c_hi)), 1.0 + U23))


def mlp_intervals(ws, x_lo, x_hi=None, block=16384):
    """ws: the f16 matrices of split_weights; inputs pinned at x_lo (f16 values) or in [x_lo, x_hi].  Returns lo / hi (n, 16) f16 of the
    output layer, act_lo / act_hi (n, 16) f16 of its sigmoid, and s / e (n, 16) float64 of the output layer where its inputs were pinned
    single values all the way (else None)."""
    n = x_lo.shape[0]
    out = SimpleNamespace(lo=np.empty((n, 16), np.float16), hi=np.empty((n, 16), np.float16), act_lo=np.empty((n, 16), np.float16),
                          act_hi=np.empty((n, 16), np.float16), n=n)
    for a in range(0, n, block):
        lo = np.asarray(x_lo[a:a + block], np.float64)
        hi = lo if x_hi is None else np.asarray(x_hi[a:a + block], np.float64)
        for i, W in enumerate(ws):
            s_lo, s_hi, e = layer_interval(W, lo, hi)
            last = i == len(ws) - 1
            l16, h16 = activation_interval(s_lo, s_hi, e, relu=not last)
            if last:
                out.lo[a:a + block], out.hi[a:a + block] = l16, h16
                out.act_lo[a:a + block], out.act_hi[a:a + block] = sigmoid_interval(s_lo - e, s_hi + e)
            else:
                lo, hi = l16.astype(np.float64), h16.astype(np.float64)
                if np.array_equal(l16, h16):
                    hi = lo
    return out


def forward_point(ws, x, relu_last=False):
    """The float64 forward with the kernel's f16 rounding points, ONE value per output: the expected bits wherever every sum is exact
    (exact nets, one-hot inputs), the midpoint of the interval elsewhere.  Returns (n, 16) f16."""
    a = np.asarray(x, np.float64)
    for i, W in enumerate(ws):
        a = f16(a @ W.astype(np.float64).T)
        if i < len(ws) - 1 or relu_last:
            a = np.maximum(a, np.float16(0)) + np.float16(0)
        a = a.astype(np.float64) if i < len(ws) - 1 else a
    return a


# SH degree 4: the kernel's f32 constants (csrc/mlp.hip sh4())
_C = [np.float64(np.float32(v)) for v in (0.28209479177387814, 0.48860251190291987, 1.0925484305920792, 0.94617469575755997,
                                          0.31539156525251999, 0.54627421529603959, 0.59004358992664352, 2.8906114426405538,
                                          0.45704579946446572, 0.3731763325901154, 1.4453057213202769)]
SH_ROUNDINGS = 32


def sh_exact(d):
    """d (n, 3) f32, un-normalised -> value, mass (n, 16) float64 of the sixteen polynomials on d / |d|."""
    d = np.asarray(d, np.float32).astype(np.float64)
    if not (np.abs(d).max(axis=1) > 0).all():
        raise ValueError("a zero direction")
    u = d / np.sqrt((d * d).sum(axis=1, keepdims=True))
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    x2, y2, z2 = x * x, y * y, z * z
    c0, c1, c2, c3, c3b, c4, c5, c6, c7, c8, c9 = _C
    one = np.ones_like(x)
    val = [c0 * one, -c1 * y, c1 * z, -c1 * x, c2 * x * y, -c2 * y * z, c3 * z2 - c3b, -c2 * x * z, c4 * x2 - c4 * y2,
           c5 * y * (-3.0 * x2 + y2), c6 * x * y * z, c7 * y * (1.0 - 5.0 * z2), c8 * z * (5.0 * z2 - 3.0), c7 * x * (1.0 - 5.0 * z2),
           c9 * z * (x2 - y2), c5 * x * (-x2 + 3.0 * y2)]
    mass = [c0 * one, c1 * ay, c1 * az, c1 * ax, c2 * ax * ay, c2 * ay * az, c3 * z2 + c3b, c2 * ax * az, c4 * x2 + c4 * y2,
            c5 * ay * (3.0 * x2 + y2), c6 * ax * ay * az, c7 * ay * (1.0 + 5.0 * z2), c8 * az * (5.0 * z2 + 3.0), c7 * ax * (1.0 + 5.0 * z2),
            c9 * az * (x2 + y2), c5 * ax * (x2 + 3.0 * y2)]
    return np.stack(val, 1), np.stack(mass, 1)


def sh_interval(d):
    """(n, 16) f16 lo, hi of the SH input chunk.  The constant term carries no rounding at all."""
    val, mass = sh_exact(d)
    e = SH_ROUNDINGS * U24 * mass
    e[:, 0] = 0.0
    return f16(val - e), f16(val + e)


def sigma_interval(h0_lo, h0_hi=None):
    """float64 lo, hi of sigma = __expf(h0) for h0 in [h0_lo, h0_hi] (f16 values), and `flush`: where 0 is accepted as well."""
    h0_lo = np.asarray(h0_lo, np.float64)
    h0_hi = h0_lo if h0_hi is None else np.asarray(h0_hi, np.float64)
    with np.errstate(over="ignore", under="ignore"):
        lo = np.exp(h0_lo) * (1.0 - (np.abs(h0_lo) + 3.0) * U23)
        hi = np.exp(h0_hi) * (1.0 + (np.abs(h0_hi) + 3.0) * U23)
        sub_lo, sub_hi = np.exp(h0_lo) < F32_MIN_NORMAL, np.exp(h0_hi) < F32_MIN_NORMAL
    lo = np.where(sub_lo, np.maximum(lo - F32_MIN_SUB, 0.0), lo)
    hi = np.where(sub_hi, hi + F32_MIN_SUB, hi)
    lo = np.where(h0_lo <= -104.0, 0.0, np.where(lo > F32_MAX, np.inf, lo))
    hi = np.where(h0_hi <= -104.0, 0.0, np.where(hi > F32_MAX, np.inf, hi))
    lo = np.where(h0_lo >= 89.0, np.inf, lo)
    return lo, hi, sub_lo


# ------------------------------------------------------------------------------------------------------------------ the check
def check(got, lo, hi, what="", also_zero=None):
    """THE check, shared by the GPU tests and the CPU mutation tests: every element of `got` inside [lo, hi] (also_zero: where an exact
    0 is accepted as well).  A NaN is outside every interval; no output is ever filtered out.  Returns bad (the number outside), n,
    share_bad, worst (a description), and, where lo / hi are f16, the share of outputs whose interval is a single f16 value and at
    most 1 and at most 4 f16 spacings wide."""
    got, lo_a, hi_a = np.asarray(got), np.asarray(lo), np.asarray(hi)
    assert got.shape == lo_a.shape == hi_a.shape, (got.shape, lo_a.shape, hi_a.shape)
    # f16 and f32 values compare exactly as f32; anything with a float64 in it as float64
    wide = np.float64 if np.float64 in (got.dtype, lo_a.dtype, hi_a.dtype) else np.float32
    g = got.astype(wide)
    res = SimpleNamespace(bad=0, n=g.size, share_bad=0.0, worst="", single=float("nan"), le1=float("nan"), le4=float("nan"))
    if g.size == 0:
        return res
    lo64, hi64 = lo_a.astype(wide), hi_a.astype(wide)
    with np.errstate(invalid="ignore"):
        inside = (g >= lo64) & (g <= hi64)
        if also_zero is not None:
            inside |= np.asarray(also_zero) & (g == 0)
    res.bad = int(inside.size - np.count_nonzero(inside))
    res.share_bad = res.bad / g.size
    if lo_a.dtype == np.float16:
        width = ord16(hi_a) - ord16(lo_a)
        assert (width >= 0).all(), "an interval with hi < lo"
        res.single, res.le1, res.le4 = float((width == 0).mean()), float((width <= 1).mean()), float((width <= 4).mean())
    if res.bad:
        with np.errstate(invalid="ignore", over="ignore"):
            below, above = np.where(g < lo64, lo64 - g, 0.0), np.where(g > hi64, g - hi64, 0.0)
            dist = np.where(inside, 0.0, np.where(np.isfinite(g) & np.isfinite(below + above), below + above, np.inf))
        i = np.unravel_index(int(np.argmax(dist)), dist.shape)
        res.worst = "%s: %d of %d outside (%.2f %%); worst at %s: got %r, interval [%r, %r]" % (
            what, res.bad, g.size, 100.0 * res.share_bad, tuple(int(v) for v in i), float(g[i]), float(lo64[i]), float(hi64[i]))
    return res


def check_sigma(got, h0_lo, h0_hi=None, what="sigma"):
    lo, hi, flush = sigma_interval(h0_lo, h0_hi)
    return check(got, lo, hi, what, also_zero=flush)


def check_rgb(got, act_lo, act_hi, what="rgb"):
    """rgb (n, 3) f32 inside its f16 interval AND an f16 value."""
    res = check(got, act_lo, act_hi, what)
    not16 = ~is_f16_value(np.asarray(got, np.float32))
    res.not_f16 = int(not16.sum())
    if res.not_f16:
        res.bad += int((not16 & (np.asarray(got, np.float64) >= act_lo.astype(np.float64)) & (np.asarray(got, np.float64) <= act_hi.astype(np.float64))).sum())
        res.share_bad = res.bad / res.n
        res.worst = (res.worst + "; " if res.worst else what + ": ") + "%d values are no f16 values" % res.not_f16
    return res


def least_ratio(got16, s, e):
    """The smallest |a - s| / e over the f32 accumulators a that round to the f16 output (the accumulator itself is not observable): 0
    where the output is f16(s) or next to it within half a spacing, above 1 exactly where the output is outside its interval."""
    g = np.asarray(got16, np.float16)
    g64 = g.astype(np.float64)
    o = ord16(g)
    up = np.where(o >= 0, o + 1, o - 1)                                  # the next f16 away from zero, as an ordinal
    bits = np.where(up >= 0, up, (-up) | 0x8000).astype(np.uint16)
    half = 0.5 * np.abs(bits.view(np.float16).astype(np.float64) - g64)
    gap = np.maximum(np.abs(g64 - s) - half, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(gap == 0, 0.0, gap / e)


# ------------------------------------------------------------------------------------------------------------------ exact nets
def exact_net(n_in, n_hidden, n, seed):
    """Dense integer-valued f16 weights (scaled by powers of two) and inputs with mass <= 2048 units in every layer.  Returns
    (blob f16, x (n, n_in) f16, expected (n, 16) f16)."""
    rng = np.random.RandomState(seed)
    dims = [n_in] + [HID] * n_hidden + [16]
    x_unit = 2.0 ** -3
    x = rng.randint(-2, 3, size=(n, n_in)).astype(np.float64) * x_unit
    # (largest integer, share of zeros, unit) per layer: dense where the sums allow it, sparser where 64-term sums of grown activations
    # would pass 2048 units
    plans = {1: [(2, 0.0, 2.0 ** -1), (1, 0.5, 2.0 ** 1)], 2: [(2, 0.0, 2.0 ** -1), (1, 0.25, 2.0 ** -2), (1, 0.75, 2.0 ** 2)]}[n_hidden]
    ws, a, unit = [], x, x_unit
    for i, (top, zeros, w_unit) in enumerate(plans):
        W = rng.randint(-top, top + 1, size=(dims[i + 1], dims[i])).astype(np.float64)
        W[rng.rand(*W.shape) < zeros] = 0
        W *= w_unit
        unit *= w_unit
        mass = np.abs(a) @ np.abs(W).T
        assert mass.max() <= 2048 * unit, "exact_net(%d, %d): layer %d has mass %g units" % (n_in, n_hidden, i, mass.max() / unit)
        s = a @ W.T
        assert np.array_equal(np.rint(s / unit), s / unit) and np.array_equal(f16(s).astype(np.float64), s)
        a = np.maximum(s, 0) + 0.0 if i < len(plans) - 1 else s + 0.0           # + 0.0: no -0 anywhere (an exact sum of zero is +0)
        ws.append(W.astype(np.float16))
        assert np.array_equal(ws[-1].astype(np.float64), W)
    blob = np.concatenate([w.reshape(-1) for w in ws])
    return blob, x.astype(np.float16), f16(a)


def exactness_holds(ws, x):
    """The condition itself, on any net: all values multiples of a power-of-two unit per layer with mass <= 2048 units."""
    a = np.asarray(x, np.float64)
    for i, W in enumerate(ws):
        W = W.astype(np.float64)
        nz = np.abs(a[:, :, None] * W.T[None]).reshape(-1)                # every product
        nz = nz[nz > 0]
        if nz.size == 0:
            return True
        unit = 2.0 ** np.floor(np.log2(nz.min()))
        while unit > 2.0 ** -40 and not np.array_equal(np.rint(nz / unit), nz / unit):
            unit /= 2
        if unit <= 2.0 ** -40 or (np.abs(a) @ np.abs(W).T).max() > 2048 * unit:
            return False
        s = a @ W.T
        a = np.maximum(s, 0) if i < len(ws) - 1 else s
    return True


# ------------------------------------------------------------------------------------------------------------------ emulation
ORDERS = ("asc", "desc", "kernel")
MUTANTS = ("truncate", "drop_first", "drop_out", "chunk_natural", "sigma_unrounded", "rgb_unrounded", "sh_unnormalised")


def d_order(c):
    """Units of chunk c in the order a D fragment hands them over: lane-half 0 first, element e -> 16c + 4hh + (e & 3) + 8(e >> 2)."""
    return [16 * c + 4 * hh + (e & 3) + 8 * (e >> 2) for hh in range(2) for e in range(8)]


def k_order(name, K, fragment_chunks):
    nat = list(range(K))
    if name == "asc":
        return nat, nat
    if name == "desc":
        return nat[::-1], nat[::-1]
    assert name == "kernel"
    o = []
    for c in range(K // 16):
        o += d_order(c) if c in fragment_chunks else nat[16 * c:16 * c + 16]
    return o, o


def chain(W, A, order, drop=None, weight_order=None):
    """acc (n, O) f32 = the k-ordered chain over f16 W (O, K) and f16 A (n, K).  weight_order (a wrong kernel): the weight column used
    at each step, where it differs from the activation's unit."""
    Wf, Af = W.astype(np.float32), A.astype(np.float32)
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j, k in enumerate(order):
            if k == drop:
                continue
            kw = k if weight_order is None else weight_order[j]
            acc = acc + Af[:, k:k + 1] * Wf[None, :, kw]             # the product is exact in f32: this is fmaf(w, a, acc)
    return acc


def _to16(acc, relu, mut):
    with np.errstate(over="ignore"):
        h = f16_trunc(acc) if mut == "truncate" else acc.astype(np.float16)
    return np.maximum(h, np.float16(0)) + np.float16(0) if relu else h          # + 0: the kernel's ReLU turns -0 into +0


def _layers(ws, x16, order, mut, first_fragment_chunks=()):
    """Through all layers; returns the f32 accumulator of the output layer (n, 16)."""
    a = np.asarray(x16, np.float16)
    for i, W in enumerate(ws):
        K = W.shape[1]
        frag = set(first_fragment_chunks) if i == 0 else set(range(K // 16))
        o, _ = k_order(order, K, frag)
        drop = None
        if (mut == "drop_first" and i == 0) or (mut == "drop_out" and i == len(ws) - 1):
            drop = o[len(o) // 2 + 1]
        worder = None
        if mut == "chunk_natural" and i == 1:
            # chunk 1 of the first layer that reads a fragment: the weights in natural order against activations in D order
            worder = [(list(range(16, 32))[d_order(1).index(k)] if 16 <= k < 32 else k) for k in o]
        acc = chain(W, a, o, drop, worder)
        if i < len(ws) - 1:
            a = _to16(acc, True, mut)
    return acc


def _sigmoid32(c32, mut):
    v = sigmoid(c32.astype(np.float64)).astype(np.float32)
    return v if mut == "rgb_unrounded" else v.astype(np.float16).astype(np.float32)


def emulate_mlp(ws, x16, order="kernel", out_act=0, mut=None):
    """ngp_mlp_fwd: (n, 16) f16."""
    acc = _layers(ws, x16, order, mut)
    return _sigmoid32(acc, mut).astype(np.float16) if out_act == 1 else _to16(acc, False, mut)


def sh4_f32(d, normalise=True):
    """The kernel's own f32 operations (contraction off), then f16: (n, 16) f16."""
    d = np.asarray(d, np.float32)
    f = np.float32
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    if normalise:
        inv = f(1.0) / np.sqrt(dx * dx + dy * dy + dz * dz)
        x, y, z = dx * inv, dy * inv, dz * inv
    else:
        x, y, z = dx, dy, dz
    c0, c1, c2, c3, c3b, c4, c5, c6, c7, c8, c9 = [f(v) for v in _C]
    xy, xz, yz, x2, y2, z2 = x * y, x * z, y * z, x * x, y * y, z * z
    o = [np.full_like(x, c0), -c1 * y, c1 * z, -c1 * x, c2 * xy, -c2 * yz, c3 * z2 - c3b, -c2 * xz, c4 * x2 - c4 * y2,
         c5 * y * (f(-3.0) * x2 + y2), c6 * xy * z, c7 * y * (f(1.0) - f(5.0) * z2), c8 * z * (f(5.0) * z2 - f(3.0)),
         c7 * x * (f(1.0) - f(5.0) * z2), c9 * z * (x2 - y2), c5 * x * (-x2 + f(3.0) * y2)]
    with np.errstate(over="ignore"):
        return np.stack(o, 1).astype(np.float16)


def emulate_field(dws, rws, feats16, dirs, order="kernel", mut=None):
    """ngp_field_fwd on row-major features (n, 32) f16: h (n, 16) f16, sigma (n,) f32, rgb (n, 3) f32."""
    acc = _layers(dws, feats16, order, mut)
    h = _to16(acc, False, mut)
    with np.errstate(over="ignore", under="ignore"):
        sigma = np.exp((acc if mut == "sigma_unrounded" else h)[:, 0].astype(np.float64)).astype(np.float32)
    x = np.concatenate([sh4_f32(dirs, normalise=mut != "sh_unnormalised"), h], 1)
    c = _layers(rws, x, order, mut, first_fragment_chunks=(1,))
    return h, sigma, _sigmoid32(c[:, :3], mut)


def colour_intervals(rws, dirs, h16):
    """rgb's f16 interval from the SH interval of dirs and pinned h (the kernel's own): act_lo / act_hi (n, 3)."""
    sh_lo, sh_hi = sh_interval(dirs)
    hp = np.asarray(h16, np.float16).astype(np.float64)
    lo = np.concatenate([sh_lo.astype(np.float64), hp], 1)
    hi = np.concatenate([sh_hi.astype(np.float64), hp], 1)
    r = mlp_intervals(rws, lo, hi)
    return r.act_lo[:, :3], r.act_hi[:, :3]
