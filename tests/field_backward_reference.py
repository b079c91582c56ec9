"""TEST INFRASTRUCTURE -- the backward of the fused MLPs of csrc/mlp.hip (mlp_bwd_kernel behind ngp_mlp_bwd, ngp_density_bwd and the
colour net's half of ngp_field_bwd_two_launches; field_bwd_kernel behind ngp_field_bwd / ngp_field_bwd_guarded) restated in numpy
float64 from its CONTRACT.  No waves, tiles or fragments in here; the forward half and every constant come from
tests/field_forward_reference.py (F), whose docstring has the model of one f32 accumulation, e = K * 2^-23 * mass.

THE CONTRACT (read from csrc/mlp.hip).
  1. Forward recompute as in F: f16 inputs and weights, f32 accumulation over the whole K, f16 activations, ReLU on hidden layers.
  2. Output gradient dy, 16 units in f16, zero for units >= n_out:
       plain, out_act 0   dL_dout as given;
       plain, out_act 1   f16(f32(dout) * (sg * (1 - sg))),  sg = 1 / (1 + __expf(-c)) on the f32 accumulator c of the output layer;
       colour, units 0..2 f16(seed * scale * sg * (1 - sg)), multiplied left to right;
       density, unit 0    f16(f32(dL_dh[0]) + seed * scale * __expf(clamp(f16(c0), -15, 15))); the other units take dL_dh as given;
                          either input may be absent (a missing dL_dh is zero, a missing seed leaves unit 0 as given);
       scale = loss_scale * (*loss_scale_dev or 1), one f32 product.
  3. Hidden layers, last to first: acc = W^T dy in f32 (K = 16 from the output layer, 64 otherwise), rounded to f16, then zeroed where
     the STORED f16 activation is not > 0 (a positive pre-activation that underflows to f16 zero passes no gradient).
  4. dL_din = f16(W0^T dh0), no mask.  The colour net produces input rows 16..31 (dL/dh) only.
  5. dW_l = sum over samples of dy_l (x) a_(l-1): products of two f16 values, exact in f32; the f32 summation order over samples,
     tiles, waves and workgroups is unspecified.  The result is partials(n_samples) rows, every one fully written (zeros where a
     workgroup had no tile); rows n_out..15 of dWo are exactly 0.
  6. Active list: n_eff = min(*n_active, n_samples); inputs, directions and f32 seeds by sample id active[j]; dL_dout16 (in) and
     dL_din (out) by compact position j; level-major planes have stride n_samples; nothing at positions >= n_eff is written.
  7. The fused kernel: dfeats bit for bit the two-launch chain; dL/dh rounded to f16 exactly where the hand-over rounded it.

THE UNDECIDED MASK.  The reference does not know the kernel's f16 hidden activation, only its interval [a_lo, a_hi] (F).  Per hidden
unit the mask is ON (a_lo > 0), OFF (a_hi == 0) or UNDECIDED; with [g_lo, g_hi] the f16 interval of the rounded W^T dy,

    on: [g_lo, g_hi]      off: [0, 0]      undecided: [min(g_lo, 0), max(g_hi, 0)]   (the hull of both outcomes).

No sample is selected or left out; an undecided unit only widens what follows it.  The same hull serves dW: where the unit is off in
the kernel its gradient AND its activation are 0, and (0, 0) is a corner of the box [g] x [a] whenever the unit is undecided.

ERROR MODEL.  Nothing but F's constants and counted roundings.
  accumulators   [s_lo - e, s_hi + e], e = K * 2^-23 * mass, through W+ / W- exactly as F.layer_interval (called on W^T), with the mass
                 taken from NOMINAL magnitudes (next paragraph).
  sg * (1 - sg)  sg' = sigmoid(c)(1 + d), |d| <= DELTA(c) (F.delta_sigmoid), so sg' in [a, b] = [sigmoid(c_lo)(1 - DELTA), min(1,
                 sigmoid(c_hi)(1 + DELTA))].  The kernel's product is p(sg') (1 + u), p(s) = s (1 - s), u the rounding of 1 - sg' (exact
                 by Sterbenz above 1/2, counted anyway).  p is not monotone: over [a, b] its minimum is at an end and its maximum is
                 1/4 where the interval holds 1/2 (which it does wherever [c_lo, c_hi] holds 0), else at an end.
  products       value * (1 + t), |t| <= R * 2^-24 * 1.001 with R the f32 roundings counted: plain out_act 1: (1 - sg), sg * (..),
                 g * (..): R = 3.  Colour: seed * scale, * sg, (1 - sg), * (..): R = 4.  (1.001 holds the second-order terms, as in F.)
  TruncExp       h0 = clamp(f16(c0)) is monotone in c0; __expf(h0) = exp(h0)(1 + a), |a| <= (|h0| + 3) 2^-23 (F.sigma_interval).  Then
                 seed * scale, * __expf, the addition: R = 3 roundings, each relative to a quantity bounded by |dL_dh0| + |product|,
                 which also covers a contracted multiply-add (one rounding fewer).
  f16            every conversion is round to nearest even, monotone: applied to both ends.
  dW             the test adds the partial rows in float64 on the host (exact to 2^-53).  Over n_eff samples and W wave slabs per
                 workgroup the f32 additions number less than n_eff + W per element in any grouping, each off by at most 2^-23 of a
                 partial sum bounded by mass = sum_s max|dy| max|a|:  [lo - B, hi + B], B = (n_eff + W [+ 31]) * 2^-23 * mass, where lo / hi
                 sum, per sample, the smallest / largest of the FOUR CORNERS of [dy] x [a].  Two exact short cuts of the four corners
                 keep that a matrix product: a pinned (lo = a+ dy_lo + a- dy_hi) and a >= 0, true of every hidden activation
                 (lo = min(dy_lo, 0) a_hi + max(dy_lo, 0) a_lo); the general case (the SH chunk of the colour net) runs in blocks.
                 The float64 evaluation is off by n * 2^-53 * mass, 2^-30 of B.

SUBNORMAL OPERANDS (a finding of the first run on an MI355X).  With mass = sum |w| |a| three of the 38
tests stopped at an output outside its interval (one dL_din value, three dW sums), all on the wide-spread weights, where weights (down to
2^-24) and hidden gradients are f16 SUBNORMALS.
The one all-pinned element was worked through by hand: dW0[34, 22] of 64-64-16 at n = 31 is a sum of ten products dh0 * x with dh0 in
{1, 2, 3, 4} * 2^-24.  The exact sum is 552.109375 * 2^-34; the device returned 552 * 2^-34: the product 2^-24 * 1031 * 2^-16 had lost
everything below 2^-37, although the largest product of the sum is only 1.05 * 2^-22 and 24 bits below THAT reach 2^-45.  It is what a
unit does that aligns the products by their operands' exponent FIELDS without normalising a subnormal first: a subnormal (and a zero)
carries the field of 2^-14, the largest nominal exponent here is that of 2^-14 * 2.67, and 24 bits below 2^-13 end at 2^-37.  The error
is still 2^-23 relative, but to the NOMINAL magnitude.  So the model was corrected by that derivation, not widened by a factor: in
every mass of this file an operand counts as  nominal(v) = max(|v|, 2^-14).  For operands that are normal f16 values nothing changes
but for the zeros (a ReLU zero adds 2^-14 |w| to a mass of order 10: 10^-5 of it).  F itself, which holds the FORWARD kernels, is left
as section 19 validated it; the forward RECOMPUTE inside this file goes through the nominal mass as well (layer_interval() below), which
is the conservative side: its activation intervals can only be wider than F's, and a few more masks undecided.
For dW the lanes behind the end of the list multiply a zero gradient with the re-read last sample: at most 31 products of nominal
magnitude 2^-14 max_s |a|, which are added to the mass and to the count of additions (n_eff + 31 + W).  On the first run after the
correction no output was outside; the largest dW error was 0.017 of B everywhere and, measured against the bound from the TRUE mass,
0.027 on the trained-like weights and 9.9 on the wide-spread ones.  tests/test_field_backward_exact_gpu.py keeps the worked element as
a case of its own (test_subnormal_operands_are_aligned_by_their_exponent_field).

EXACT NETS (exact_backward_net()).  F.exact_net() with dL_dout in {-2..2} * 2^-4: every dgrad mass <= 2048 units (f16 holds every
partial sum), every dW mass <= 2^24 units (f32 does): any order gives the same bits and backward_point() is THE expected value.

EMULATION (emulate_backward / emulate_field_backward).  One launch in plain f32 numpy, natural K order, tile t on workgroup
(t mod (grid * W)) div W; `mut` names a deliberately wrong kernel (MUTANTS) for tests/test_field_backward_reference_cpu.py.  It is
NOT pinned on the device: DESIGN.md section 19 found that the MFMA is no k-ordered chain."""
from types import SimpleNamespace

import numpy as np

from tests import field_forward_reference as F

U23, U24, HID, TILE = F.U23, F.U24, F.HID, F.TILE
R_PLAIN_ACT, R_COLOUR, R_DENSITY = 3, 4, 3
NAN16 = np.uint16(0x7E5A).view(np.float16)
NAN32 = np.uint32(0x7FC5A5A5).view(np.float32)


# ------------------------------------------------------------------------------------------------------------------ launch geometry
def waves(n_in, n_hidden, fused=False):
    """Waves per workgroup of the instantiation (bwd_waves() of csrc/mlp.hip; field_bwd_kernel has 4)."""
    return 4 if fused or n_in > 32 or n_hidden == 2 else 8


def partials(n_samples):
    """ngp_mlp_bwd_partials / ngp_field_bwd_partials."""
    if n_samples <= 0:
        return 0
    tiles = -(-n_samples // TILE)
    return max(1, min(256, -(-tiles // 4)))


def sweep(w):
    return 256 * w * TILE


def net_size(n_in, n_hidden):
    return HID * n_in + (n_hidden - 1) * HID * HID + 16 * HID


def scale32(loss_scale, loss_scale_dev=None):
    return float(np.float32(loss_scale) * np.float32(1.0 if loss_scale_dev is None else loss_scale_dev))


def _f64(a):
    return np.asarray(a, np.float64)


F16_MIN_NORMAL = 2.0 ** -14


def nominal(v):
    """|v|, but 2^-14 for zero and every f16 subnormal: the magnitude the matrix unit aligns a product by (docstring, SUBNORMAL OPERANDS)."""
    return np.maximum(np.abs(v), F16_MIN_NORMAL)


def layer_interval(W, lo, hi):
    """F.layer_interval with e from the NOMINAL mass."""
    s_lo, s_hi, _ = F.layer_interval(W, lo, hi)
    mass = nominal(np.maximum(np.abs(lo), np.abs(hi))) @ nominal(W.astype(np.float64)).T
    return s_lo, s_hi, W.shape[1] * U23 * mass


def _pair(lo16, hi16):
    lo, hi = lo16.astype(np.float64), hi16.astype(np.float64)
    return (lo, lo) if np.array_equal(lo16, hi16) else (lo, hi)


# ------------------------------------------------------------------------------------------------------------------ output gradients
def dsigmoid_range(c_lo, c_hi):
    """float64 lo, hi of p(sg') = sg'(1 - sg') over the kernel's sigmoid of an accumulator in [c_lo, c_hi]."""
    a = F.sigmoid(c_lo) * (1.0 - F.delta_sigmoid(c_lo))
    b = np.minimum(F.sigmoid(c_hi) * (1.0 + F.delta_sigmoid(c_hi)), 1.0)
    pa, pb = a * (1.0 - a), b * (1.0 - b)
    return np.minimum(pa, pb), np.where((a <= 0.5) & (b >= 0.5), 0.25, np.maximum(pa, pb))


def _times(x, q_lo, q_hi, roundings):
    """x * [q_lo, q_hi] (q >= 0) through `roundings` f32 roundings -> f16 lo, hi."""
    v1, v2 = x * q_lo, x * q_hi
    lo, hi = np.minimum(v1, v2), np.maximum(v1, v2)
    t = roundings * U24 * 1.001
    return F.f16(lo - np.abs(lo) * t), F.f16(hi + np.abs(hi) * t)


def plain_dy(dout16, n_out, out_act):
    """dy-spec of ngp_mlp_bwd: dout16 (n, n_out) f16 by compact position."""
    def dy(c_lo, c_hi):
        n = c_lo.shape[0]
        lo = np.zeros((n, 16), np.float16)
        lo[:, :n_out] = dout16[:, :n_out]
        if out_act == 0:
            return lo, lo
        hi = lo.copy()
        q_lo, q_hi = dsigmoid_range(c_lo[:, :n_out], c_hi[:, :n_out])
        lo[:, :n_out], hi[:, :n_out] = _times(dout16[:, :n_out].astype(np.float64), q_lo, q_hi, R_PLAIN_ACT)
        return lo, hi
    return dy


def colour_dy(seed_rgb, scale):
    """dy-spec of the colour net: seed_rgb (n, 3) f32 (dL_drgbs of the listed samples), scale = scale32(...)."""
    def dy(c_lo, c_hi):
        lo = np.zeros((c_lo.shape[0], 16), np.float16)
        hi = lo.copy()
        q_lo, q_hi = dsigmoid_range(c_lo[:, :3], c_hi[:, :3])
        lo[:, :3], hi[:, :3] = _times(_f64(np.asarray(seed_rgb, np.float32)) * scale, q_lo, q_hi, R_COLOUR)
        return lo, hi
    return dy


def density_dy(dh_lo, dh_hi, seed_sigma, scale):
    """dy-spec of the density net: dL/dh pinned (dh_hi None), an f16 interval, or absent (None); seed_sigma (n,) f32 or None."""
    def dy(c_lo, c_hi):
        n = c_lo.shape[0]
        lo = np.zeros((n, 16), np.float16) if dh_lo is None else np.array(dh_lo, np.float16)
        hi = lo.copy() if dh_hi is None else np.array(dh_hi, np.float16)
        if seed_sigma is None:
            return lo, hi
        h_lo = np.clip(F.f16(c_lo[:, 0]).astype(np.float64), -15.0, 15.0)
        h_hi = np.clip(F.f16(c_hi[:, 0]).astype(np.float64), -15.0, 15.0)
        e_lo, e_hi, _ = F.sigma_interval(h_lo, h_hi)
        x = _f64(np.asarray(seed_sigma, np.float32)) * scale
        p_lo, p_hi = np.minimum(x * e_lo, x * e_hi), np.maximum(x * e_lo, x * e_hi)
        g_lo, g_hi = lo[:, 0].astype(np.float64), hi[:, 0].astype(np.float64)
        err = R_DENSITY * U24 * 1.001 * (np.maximum(np.abs(g_lo), np.abs(g_hi)) + np.maximum(np.abs(p_lo), np.abs(p_hi)))
        lo[:, 0], hi[:, 0] = F.f16(g_lo + p_lo - err), F.f16(g_hi + p_hi + err)
        return lo, hi
    return dy


# ------------------------------------------------------------------------------------------------------------------ intervals
def forward_intervals(ws, x_lo, x_hi):
    """[(lo, hi)] float64 of the network input and every hidden activation, and the output accumulator's c_lo, c_hi (n, 16)."""
    lo = _f64(x_lo)
    hi = lo if x_hi is None else _f64(x_hi)
    acts = [(lo, hi)]
    for i, W in enumerate(ws):
        s_lo, s_hi, e = layer_interval(W, lo, hi)
        if i == len(ws) - 1:
            return acts, s_lo - e, s_hi + e
        lo, hi = _pair(*F.activation_interval(s_lo, s_hi, e, relu=True))
        acts.append((lo, hi))


def _corner_sums(g_lo, g_hi, a_lo, a_hi, block=256):
    """sum over samples of the smallest / largest corner of [g] x [a], and of max|g| max|a|: (O, K) float64 each."""
    mass = nominal(np.maximum(np.abs(g_lo), np.abs(g_hi))).T @ nominal(np.maximum(np.abs(a_lo), np.abs(a_hi)))
    if a_lo is a_hi or np.array_equal(a_lo, a_hi):
        ap, an = np.maximum(a_lo, 0), np.minimum(a_lo, 0)
        return g_lo.T @ ap + g_hi.T @ an, g_hi.T @ ap + g_lo.T @ an, mass
    if (a_lo >= 0).all():
        return (np.minimum(g_lo, 0).T @ a_hi + np.maximum(g_lo, 0).T @ a_lo,
                np.maximum(g_hi, 0).T @ a_hi + np.minimum(g_hi, 0).T @ a_lo, mass)
    lo, hi = np.zeros_like(mass), np.zeros_like(mass)
    for s in range(0, g_lo.shape[0], block):
        gl, gh = g_lo[s:s + block, :, None], g_hi[s:s + block, :, None]
        al, ah = a_lo[s:s + block, None, :], a_hi[s:s + block, None, :]
        c = (gl * al, gl * ah, gh * al, gh * ah)
        lo += np.minimum(np.minimum(c[0], c[1]), np.minimum(c[2], c[3])).sum(axis=0)
        hi += np.maximum(np.maximum(c[0], c[1]), np.maximum(c[2], c[3])).sum(axis=0)
    return lo, hi, mass


def dw_intervals(g, a, counts, w):
    """{count: (lo, hi)} (O, K) float64, error term included, for every count (a prefix of the samples) from ONE cumulative pass."""
    out, lo, hi, mass, start, top = {}, 0.0, 0.0, 0.0, 0, 0.0
    for c in sorted(set(counts)):
        if c > start:
            sl = slice(start, c)
            l, h, m = _corner_sums(g[0][sl], g[1][sl], a[0][sl], a[1][sl])
            top = np.maximum(top, nominal(np.maximum(np.abs(a[0][sl]), np.abs(a[1][sl]))).max(axis=0))
            lo, hi, mass, start = lo + l, hi + h, mass + m, c
        # lanes past the end of the list: at most TILE - 1 products 0 * a, of nominal magnitude 2^-14 * |a|
        b = (c + TILE - 1 + w) * U23 * (mass + (TILE - 1) * F16_MIN_NORMAL * top[None, :])
        out[c] = (lo - b, hi + b) if c > 0 else (np.zeros((g[0].shape[1], a[0].shape[1])),) * 2
    return out


def mlp_backward_intervals(ws, x_lo, x_hi, dy, w, counts=None, din_rows=None):
    """ws: F.split_weights; network inputs of the listed samples in compact order, pinned at x_lo (x_hi None) or in [x_lo, x_hi];
    dy: a dy-spec (plain_dy / colour_dy / density_dy); w: waves per workgroup; counts: the n_eff for which dW is wanted (prefixes);
    din_rows: the input rows that dL_din holds (the colour net: 16..31).  Returns din_lo / din_hi (n, rows) f16, dw[count] = (lo, hi)
    float64 over the tight blob, dy_lo / dy_hi, and the mask statistics (hidden, undecided)."""
    n = np.asarray(x_lo).shape[0]
    counts = (n,) if counts is None else tuple(counts)
    acts, c_lo, c_hi = forward_intervals(ws, x_lo, x_hi)
    dy_lo, dy_hi = dy(c_lo, c_hi)
    g = _pair(dy_lo, dy_hi)
    grads = [None] * len(ws)
    grads[-1] = g
    hidden = undecided = 0
    zero = np.float16(0)
    for l in range(len(ws) - 1, 0, -1):
        s_lo, s_hi, e = layer_interval(ws[l].T, g[0], g[1])
        g_lo, g_hi = F.f16(s_lo - e), F.f16(s_hi + e)
        if not (np.isfinite(g_lo.astype(np.float32)).all() and np.isfinite(g_hi.astype(np.float32)).all()):
            raise ValueError("a hidden gradient beyond the f16 range: outside what the intervals cover")
        on, off = acts[l][0] > 0, acts[l][1] == 0
        g_lo = np.where(on, g_lo, np.where(off, zero, np.minimum(g_lo, zero)))
        g_hi = np.where(on, g_hi, np.where(off, zero, np.maximum(g_hi, zero)))
        hidden += on.size
        undecided += int((~on & ~off).sum())
        g = _pair(g_lo, g_hi)
        grads[l - 1] = g
    W0 = ws[0] if din_rows is None else ws[0][:, din_rows]
    s_lo, s_hi, e = layer_interval(W0.T, g[0], g[1])
    per_layer = [dw_intervals(grads[l], acts[l], counts, w) for l in range(len(ws))]
    cat = lambda c, i: np.concatenate([p[c][i].reshape(-1) for p in per_layer])
    dw = {c: (cat(c, 0), cat(c, 1)) for c in counts}
    mass = [np.maximum(np.abs(grads[l][0]), np.abs(grads[l][1])).T @ np.maximum(np.abs(acts[l][0]), np.abs(acts[l][1])) for l in range(len(ws))]   # (the true mass: for the statistics)
    return SimpleNamespace(din_lo=F.f16(s_lo - e), din_hi=F.f16(s_hi + e), dw=dw, dy_lo=dy_lo, dy_hi=dy_hi, hidden=hidden,
                           undecided=undecided, n=n, mass=np.concatenate([m.reshape(-1) for m in mass]))


# ---- the field ------------------------------------------------------------------------------------------------------------------------
def colour_backward_intervals(rws, dirs, h_lo, h_hi, seed_rgb, scale, counts=None):
    """The colour net (mlp_bwd_kernel<32, 2, IN_SH_H, OUT_RGB> or the colour half of field_bwd_kernel): input = SH interval of dirs
    and h pinned (h_hi None) or an f16 interval; din = dL/dh (n, 16)."""
    sh_lo, sh_hi = F.sh_interval(dirs)
    h_hi = h_lo if h_hi is None else h_hi
    lo = np.concatenate([sh_lo, np.asarray(h_lo, np.float16)], 1).astype(np.float64)
    hi = np.concatenate([sh_hi, np.asarray(h_hi, np.float16)], 1).astype(np.float64)
    return mlp_backward_intervals(rws, lo, hi, colour_dy(seed_rgb, scale), 4, counts, din_rows=slice(16, 32))


def density_backward_intervals(dws, feats16, dh_lo, dh_hi, seed_sigma, scale, w=8, counts=None):
    """The density net from row-major f16 features of the listed samples: din = dfeats (n, 32) row-major."""
    return mlp_backward_intervals(dws, feats16, None, density_dy(dh_lo, dh_hi, seed_sigma, scale), w, counts)


def field_backward_intervals(dws, rws, feats16, dirs, seed_sigma, seed_rgb, scale, counts=None):
    """field_bwd_kernel: everything propagated from the features.  Returns (density result, colour result)."""
    _, c_lo, c_hi = forward_intervals(dws, feats16, None)
    col = colour_backward_intervals(rws, dirs, F.f16(c_lo), F.f16(c_hi), seed_rgb, scale, counts)
    return density_backward_intervals(dws, feats16, col.din_lo, col.din_hi, seed_sigma, scale, 4, counts), col


# ------------------------------------------------------------------------------------------------------------------ the point value
def backward_point(ws, x, dy, counts=None, din_rows=None):
    """The float64 backward with the kernel's f16 rounding points and masks from the f16 activations, ONE value per output: the
    expected value wherever every sum is exact.  dy: (n, 16) f16, or a function of the output pre-activation c (n, 16) float64.
    Returns din (n, rows) f16 and dw[count] float64 over the tight blob."""
    a = _f64(x)
    acts = [a]
    for W in ws[:-1]:
        a = np.maximum(F.f16(a @ W.astype(np.float64).T), np.float16(0)).astype(np.float64)
        acts.append(a)
    g = _f64(dy(a @ ws[-1].astype(np.float64).T) if callable(dy) else dy)
    grads = [None] * len(ws)
    grads[-1] = g
    for l in range(len(ws) - 1, 0, -1):
        g = np.where(acts[l] > 0, F.f16(g @ ws[l].astype(np.float64)).astype(np.float64), 0.0)
        grads[l - 1] = g
    W0 = ws[0] if din_rows is None else ws[0][:, din_rows]
    din = F.f16(g @ W0.astype(np.float64)) + np.float16(0)
    counts = (a.shape[0],) if counts is None else tuple(counts)
    dw, acc, start = {}, [np.zeros((grads[l].shape[1], acts[l].shape[1])) for l in range(len(ws))], 0
    for c in sorted(set(counts)):
        for l in range(len(ws)):
            acc[l] = acc[l] + grads[l][start:c].T @ acts[l][start:c]
        start = max(start, c)
        dw[c] = np.concatenate([m.reshape(-1) for m in acc])
    return din, dw


def pad16(dout16, n_out):
    out = np.zeros((dout16.shape[0], 16), np.float16)
    out[:, :n_out] = dout16[:, :n_out]
    return out


def density_point_dy(dh16, seed_sigma, scale):
    def dy(c):
        g = np.zeros((c.shape[0], 16)) if dh16 is None else dh16.astype(np.float64)
        if seed_sigma is not None:
            h0 = np.clip(F.f16(c[:, 0]).astype(np.float64), -15.0, 15.0)
            g[:, 0] = g[:, 0] + _f64(np.asarray(seed_sigma, np.float32)) * scale * np.exp(h0)
        return F.f16(g)
    return dy


# ------------------------------------------------------------------------------------------------------------------ exact nets
def assert_backward_exact(ws16, x, dy, dy_unit):
    """The exactness condition of a backward: dy (n, 16) multiples of dy_unit; every dgrad mass <= 2048 units, every dW mass <= 2^24."""
    ws = [w.astype(np.float64) for w in ws16]
    d, unit = np.asarray(dy, np.float64), dy_unit

    def unit_of(v):
        nz = np.abs(v[v != 0])
        u = 2.0 ** np.floor(np.log2(nz.min())) if nz.size else 1.0
        while nz.size and not np.array_equal(np.rint(nz / u), nz / u):
            u /= 2
        return u
    a = np.asarray(x, np.float64)
    acts = [a]
    for W in ws[:-1]:
        a = np.maximum(a @ W.T, 0)
        acts.append(a)
    g, gu = d, unit
    for l in range(len(ws) - 1, -1, -1):
        mass = np.abs(g).T @ np.abs(acts[l])
        assert mass.max() <= 2.0 ** 24 * gu * unit_of(acts[l]), "dW%d has mass %g units" % (l, mass.max() / (gu * unit_of(acts[l])))
        gu *= unit_of(ws[l])
        mass = np.abs(g) @ np.abs(ws[l])
        assert mass.max() <= 2048 * gu, "dgrad through layer %d has mass %g units" % (l, mass.max() / gu)
        s = g @ ws[l]
        assert np.array_equal(F.f16(s).astype(np.float64), s)
        g = np.where(acts[l] > 0, s, 0.0) if l > 0 else s


def exact_backward_net(n_in, n_hidden, n, seed, nonzero_rows=None):
    """F.exact_net() plus dL_dout (n, 16) in {-2..2} * 2^-4 (zero outside nonzero_rows); asserts that every dgrad mass is <= 2048
    units and every dW mass <= 2^24 units, for every n_out (masses only shrink with fewer output units).  Returns blob, x, dout."""
    blob, x, _ = F.exact_net(n_in, n_hidden, n, seed)
    rng = np.random.RandomState(seed + 9000)
    unit = 2.0 ** -4
    d = rng.randint(-2, 3, size=(n, 16)).astype(np.float64) * unit
    if nonzero_rows is not None:
        keep = np.zeros(n, bool)
        keep[nonzero_rows] = True
        d[~keep] = 0
    d = d + 0.0
    assert_backward_exact(F.split_weights(blob, n_in, n_hidden), x, d, unit)
    return blob, x, d.astype(np.float16)


# ------------------------------------------------------------------------------------------------------------------ emulation
MUTANTS = ("drop_tail_tile", "clamped_lanes_add", "mask_wrong_layer", "truncate_dh", "dout_by_sample_id", "seeds_by_position",
           "dwo_from_h0", "no_dsigmoid", "scale_twice", "no_clamp", "stride_n_eff", "idle_row_unwritten", "one_launch_density_dw_tail")


def _chain16(W, a16):
    return F.chain(W, a16, range(W.shape[1]))


def _sg32(c32):
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-c32.astype(np.float64)).astype(np.float32))).astype(np.float32)


def emulate_backward(family, ws, inputs, n_samples, w, dout=None, n_out=16, out_act=0, seed=None, scale=1.0, active=None, n_active=None,
                     dirs=None, mut=None):
    """One launch of mlp_bwd_kernel.  family "plain": inputs (n_samples, n_in) f16, dout (>= n_eff, n_out) f16; "density": inputs =
    row-major features (n_samples, 32), dout = dL/dh (>= n_eff, 16) or None, seed (n_samples,) f32 or None; "colour": inputs = h
    (n_samples, 16), dirs (n_samples, 3), seed (n_samples, 3).  Returns din over a NaN prefill -- plain (n_samples, n_in), density
    level-major (16, n_samples, 2), colour (n_samples, 16) -- and the partial rows (partials(n_samples), net size) f32."""
    f32 = np.float32
    n_eff = n_samples if active is None else max(0, min(int(n_active), n_samples))
    ids = np.arange(n_eff) if active is None else np.clip(np.asarray(active[:n_eff], np.int64), 0, n_samples - 1)
    pos = np.arange(n_eff)
    x = np.asarray(inputs, np.float16)[ids]
    if family == "colour":
        x = np.concatenate([F.sh4_f32(np.asarray(dirs, np.float32)[ids]), x], 1)
    acts = [x]
    for W in ws[:-1]:
        acts.append(F._to16(_chain16(W, acts[-1]), True, None))
    c = _chain16(ws[-1], acts[-1])
    sd = None if seed is None else np.asarray(seed, np.float32)[pos if mut == "seeds_by_position" else ids]
    s32 = f32(scale) * (f32(scale) if mut == "scale_twice" else f32(1))
    dy = np.zeros((n_eff, 16), np.float16)
    with np.errstate(over="ignore", invalid="ignore"):
        if family == "colour":
            sg = _sg32(c[:, :3])
            v = sd * s32
            dy[:, :3] = (v if mut == "no_dsigmoid" else v * sg * (f32(1) - sg)).astype(np.float16)
        else:
            g = np.zeros((n_eff, 16), f32)
            if dout is not None:
                cols = 16 if family == "density" else n_out
                g[:, :cols] = np.asarray(dout, np.float16)[ids if mut == "dout_by_sample_id" else pos][:, :cols].astype(f32)
            if family == "density":
                if sd is not None:
                    h0 = c[:, 0].astype(np.float16).astype(f32)
                    if mut != "no_clamp":
                        h0 = np.clip(h0, f32(-15), f32(15))
                    g[:, 0] = g[:, 0] + sd * s32 * np.exp(h0.astype(np.float64)).astype(f32)
            elif out_act == 1 and mut != "no_dsigmoid":
                sg = _sg32(c)
                g = g * (sg * (f32(1) - sg))
                g[:, n_out:] = 0
            dy = g.astype(np.float16)
    grads = [None] * len(ws)
    grads[-1] = dy
    for l in range(len(ws) - 1, 0, -1):
        acc = _chain16(ws[l].T, grads[l])
        with np.errstate(over="ignore"):
            d16 = F.f16_trunc(acc) if mut == "truncate_dh" else acc.astype(np.float16)
        mask_of = (len(ws) - l) if (mut == "mask_wrong_layer" and len(ws) == 3) else l
        grads[l - 1] = np.where(acts[mask_of] > 0, d16, np.float16(0))
    rows = slice(16, 32) if family == "colour" else slice(None)
    with np.errstate(over="ignore"):
        din = _chain16(ws[0][:, rows].T, grads[0]).astype(np.float16)
    # ---- dL_din by compact position
    if family == "density":
        buf = np.full(16 * n_samples * 2, NAN16, np.float16)
        stride = n_eff if mut == "stride_n_eff" else n_samples
        if n_eff:
            lvl = np.arange(16)[:, None, None]
            idx = (lvl * stride + pos[None, :, None]) * 2 + np.arange(2)[None, None, :]
            buf[idx] = din.reshape(n_eff, 16, 2).transpose(1, 0, 2)
        buf = buf.reshape(16, n_samples, 2)
    else:
        buf = np.full((n_samples, din.shape[1]), NAN16, np.float16)
        buf[:n_eff] = din
    # ---- dW partial rows: tile t on workgroup (t mod (grid * w)) div w, 32-sample sums added in tile order
    grid = partials(n_samples)
    part = np.full((grid, sum(W.size for W in ws)), NAN32, np.float32)
    n_tiles = -(-n_eff // TILE)
    busy = {(t % (grid * w)) // w for t in range(n_tiles)}
    for b in range(grid):
        if b in busy or mut != "idle_row_unwritten":
            part[b] = 0
    src = [acts[l] if not (mut == "dwo_from_h0" and l == len(ws) - 1 and len(ws) == 3) else acts[1] for l in range(len(ws))]
    offs = np.cumsum([0] + [W.size for W in ws])
    for t in range(n_tiles):
        b = (t % (grid * w)) // w
        sl = np.arange(t * TILE, min((t + 1) * TILE, n_eff))
        if sl.size < TILE:
            if mut == "drop_tail_tile":
                continue
            if mut == "clamped_lanes_add":
                sl = np.concatenate([sl, np.full(TILE - sl.size, n_eff - 1)])
        with np.errstate(invalid="ignore", over="ignore"):            # (a wrong kernel's rows may hold the NaN prefill or an inf)
            for l in range(len(ws)):
                part[b, offs[l]:offs[l + 1]] += (grads[l][sl].astype(f32).T @ src[l][sl].astype(f32)).reshape(-1)
    return buf, part


def emulate_field_backward(dws, rws, feats16, dirs, seed_sigma, seed_rgb, scale, n_samples, active=None, n_active=None, mut=None):
    """field_bwd_kernel as its two-launch chain (4 waves each): dfeats level-major, density rows, colour rows, and the two hand-overs
    that stay in registers, dL/dh (n_samples, 16) by compact position and h (n_samples, 16) by sample id.  The wrong kernel
    "one_launch_density_dw_tail" is wrong ONLY in the density net's dW (its last partial tile is missing): the one-launch kernel's
    weight-gradient code is its own."""
    dmut = "drop_tail_tile" if mut == "one_launch_density_dw_tail" else mut
    h = _chain16(dws[-1], F._to16(_chain16(dws[0], np.asarray(feats16, np.float16)), True, None)).astype(np.float16)
    dh, part_r = emulate_backward("colour", rws, h, n_samples, 4, seed=seed_rgb, scale=scale, active=active, n_active=n_active, dirs=dirs,
                                  mut=mut)
    n_eff = n_samples if active is None else max(0, min(int(n_active), n_samples))
    dfeats, part_d = emulate_backward("density", dws, feats16, n_samples, 4, dout=np.where(np.arange(n_samples)[:, None] < n_eff, dh, np.float16(0)),
                                      seed=seed_sigma, scale=scale, active=active, n_active=n_active, mut=dmut)
    return dfeats, part_d, part_r, dh, h
