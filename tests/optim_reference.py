"""Plain numpy float64 restatements of the optimizer, loss and AMP kernels of ngp_pl_amd/csrc/optim.hip (with adam_common.h and
loss_common.h), and the error bounds inside which a correct float32 kernel must land.  No torch, no GPU.

Every bound is a running first-order error analysis of the kernel's own expression tree:

  E    = 2^-24    unit roundoff of one float32 operation (+, -, *, and the correctly rounded / and sqrt the library is built with)
  TINY = 2^-126   absolute error of one operation whose result is flushed (or not) below the normal range

An operation's result r carries |error| <= E |r| + TINY on top of the propagated errors of its inputs.  A fused multiply-add rounds
once where the separate operations round twice, so a bound that counts every operation holds under any contraction.  The counts
below are the first-order counts k of roundings on the path of a term, written as (k + 1) E: the extra unit covers every
higher-order product of the roundings (each below k^2 E^2 < 2^-19 E for the k <= 5 that occur).  No constant is fitted to a
device result.  tests/test_optim_reference_cpu.py evaluates the same expressions in uncontracted numpy float32 and shows that
they stay inside the bounds on every case the GPU test uses.

The only measured numbers are the two absolute errors of the device logarithms, TAU_FAST (`__logf`, ngp_nerf_loss) and TAU_LOGF
(`logf`, the terms kernels): see MEASURED_TAU_FAST below."""
import numpy as np

E = 2.0 ** -24
TINY = 2.0 ** -126
F16_MAX = 65504.0

f32 = np.float32
f64 = np.float64


def ulp32(x):
    """Spacing of float32 at |x| (float64 array)."""
    x = np.abs(np.asarray(x, f32))
    return (np.nextafter(x, f32(np.inf)) - x).astype(f64)


# ------------------------------------------------------------------------------------------------------------------------------
# Adam
# ------------------------------------------------------------------------------------------------------------------------------

class AdamCoef:
    """The float32 coefficients as the launcher (adam_hyper, optim.hip) and the kernel form them:
    1 - beta (float32 subtraction, in the kernel), inv_scale = fl32(1 / grad_scale), bc_k = fl32(1 - fl32(powf(beta_k, t))).
    Held as float64 numbers that are exactly float32 values.

    d_bc1 / d_bc2: relative uncertainty of the bias corrections between two libm builds.  If powf(beta, t) differs by one ulp of
    beta^t, fl32(1 - pw) moves by at most ulp32(pw) plus one spacing of the difference (both results are rounded): relative
    ulp32(pw) / bc + 2 E."""

    def __init__(self, lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-15, wd=0.0, step=1, grad_scale=1.0):
        self.lr, self.beta1, self.beta2, self.eps, self.wd = (float(f32(x)) for x in (lr, beta1, beta2, eps, wd))
        self.step, self.grad_scale = int(step), float(f32(grad_scale))
        self.omb1 = float(f32(1) - f32(beta1))
        self.omb2 = float(f32(1) - f32(beta2))
        self.inv_scale = float(f32(1) / f32(grad_scale))
        pw1 = np.power(f32(beta1), f32(step), dtype=f32)
        pw2 = np.power(f32(beta2), f32(step), dtype=f32)
        self.pw1, self.pw2 = float(pw1), float(pw2)
        self.bc1 = float(f32(1) - pw1)
        self.bc2 = float(f32(1) - pw2)
        self.d_bc1 = float(ulp32(pw1)) / self.bc1 + 2 * E
        self.d_bc2 = float(ulp32(pw2)) / self.bc2 + 2 * E

    def launch_args(self):
        """(lr, beta1, beta2, eps, weight_decay, step, grad_scale) of the C ABI."""
        return (self.lr, self.beta1, self.beta2, self.eps, self.wd, self.step, self.grad_scale)


def adam_ref(p, m, v, g_raw, coef, e_g_raw=0.0):
    """One decoupled-weight-decay Adam step (adam_one, adam_common.h; apex FusedAdam with adam_w_mode) in float64 on float32
    inputs.  g_raw is the gradient as stored (loss-scaled); e_g_raw an absolute error bound it already carries (a float32 column
    sum, reduce_bound), 0 for a stored gradient.

        g   = g_raw * inv_scale
        m'  = beta1 m + (1 - beta1) g
        v'  = beta2 v + (1 - beta2) g g
        den = sqrt(v' / bc2) + eps
        u   = (m' / bc1) / den
        p'  = p - lr (u + wd p)

    Returns (p', m', v') and (e_p, e_m, e_v).  Roundings on each path (first-order count, + 1 as the module docstring says):

        g        1 (the product, counted on the paths below);  e_g = inv_scale e_g_raw
        beta1 m  product, sum: 2 -> 3.   (1-beta1) g: g, product, sum: 3 -> 4.
                 e_m = E (3 |beta1 m| + 4 |(1-beta1) g|) + (1-beta1) e_g + 3 TINY
        v'       beta2 v: 2;  ((1-beta2) g) g: g twice, two products, sum: 5.  All terms are >= 0, so <= 5 -> 6 E v'.
                 e_v = 6 E v' + (1-beta2) (2 |g| e_g + e_g^2) + 3 TINY
        den      s = sqrt(v'/bc2) moves by at most the width of the interval sqrt((v' +- e_v)/bc2) (exact, not linearised: v' may
                 be 0), the quotient, the root and the sum round once each (the quotient's rounding is halved by the root:
                 2.5 -> 3):   e_den = width + 3 E den + TINY.  eps keeps den far above e_den (asserted), so
                 rel_den = e_den / (den - e_den).
        u        two quotients: 2 -> 3;   e_u = (e_m / bc1) / (den - e_den) + |u| (rel_den + 3 E + d_bc1 + d_bc2 / 2) + 3 TINY
                 (d_bc: AdamCoef; the root halves bc2's)
        p'       wd p: product, sum, product by lr, difference: 4.  u: sum, product, difference: 3.  p' itself: 1 -> 2.
                 e_p = lr e_u + E (2 |p'| + 3 lr |u| + 4 lr wd |p|) + 3 TINY"""
    c = coef
    p, m, v, g_raw = (np.asarray(a, f64) for a in (p, m, v, g_raw))
    e_g_raw = np.asarray(e_g_raw, f64)
    g = g_raw * c.inv_scale
    e_g = c.inv_scale * e_g_raw
    a, b = c.beta1 * m, c.omb1 * g
    m2 = a + b
    e_m = E * (3 * np.abs(a) + 4 * np.abs(b)) + c.omb1 * e_g + 3 * TINY
    v2 = c.beta2 * v + c.omb2 * g * g
    e_v = 6 * E * v2 + c.omb2 * (2 * np.abs(g) * e_g + e_g * e_g) + 3 * TINY
    s = np.sqrt(v2 / c.bc2)
    den = s + c.eps
    width = np.sqrt((v2 + e_v) / c.bc2) - np.sqrt(np.maximum(v2 - e_v, 0.0) / c.bc2)
    e_den = width + 3 * E * den + TINY
    assert np.all(den > 4 * e_den), "eps no longer dominates the denominator's error: the bound's quotient rule does not hold"
    rel_den = e_den / (den - e_den)
    u = (m2 / c.bc1) / den
    e_u = (e_m / c.bc1) / (den - e_den) + np.abs(u) * (rel_den + 3 * E + c.d_bc1 + 0.5 * c.d_bc2) + 3 * TINY
    p2 = p - c.lr * (u + c.wd * p)
    e_p = c.lr * e_u + E * (2 * np.abs(p2) + 3 * c.lr * np.abs(u) + 4 * c.lr * c.wd * np.abs(p)) + 3 * TINY
    return (p2, m2, v2), (e_p, e_m, e_v)


def adam_f32(p, m, v, g_raw, coef):
    """adam_one evaluated in numpy float32, one rounding per operation (no contraction): what a correct kernel computes when the
    compiler fuses nothing."""
    c = coef
    p, m, v, g_raw = (np.asarray(a, f32) for a in (p, m, v, g_raw))
    b1, b2, lr, eps, wd, bc1, bc2 = (f32(x) for x in (c.beta1, c.beta2, c.lr, c.eps, c.wd, c.bc1, c.bc2))
    with np.errstate(under="ignore"):
        gk = g_raw * f32(c.inv_scale)
        m2 = b1 * m + (f32(1) - b1) * gk
        v2 = b2 * v + (f32(1) - b2) * gk * gk
        den = np.sqrt(v2 / bc2) + eps
        p2 = p - lr * ((m2 / bc1) / den + wd * p)
    return p2, m2, v2


def clamp_f16_grad(g16):
    """The f16 gradient as adam_dense reads it: fminf(fmaxf(g, -65504), 65504).  +-inf become +-65504.  NaN has two legal
    images (fmaxf / fminf may return either operand's side): callers accept the reference at +65504 or at -65504."""
    g = np.asarray(g16, np.float16).astype(f64)
    nan = np.isnan(g)
    return np.clip(np.where(nan, F16_MAX, g), -F16_MAX, F16_MAX), nan


def reduce_bound(rows, extra):
    """Error bound of a float32 column sum of `rows` (n_partials, n) against the float64 sum: every value passes through at most
    ceil(n_partials / 8) additions of its row lane's serial chain, then the lane accumulators and the 8 row lanes are combined in
    at most `extra` further additions (9 for adam_from_partials: a0 + a1 and 8 lanes; 10 for reduce_partials2_kernel:
    (a0 + a1) + (a2 + a3) and 8 lanes):  (ceil(n_partials / 8) + extra) E sum |x|."""
    rows = np.asarray(rows, f64)
    k = -(-rows.shape[0] // 8) + extra
    return k * E * np.abs(rows).sum(0)


def merge_gradient(partial, offsets, k_split, part_off):
    """The gradient adam_dense<F16_MERGE> forms below value_end: per entry, the float32 sum of the level's K partial tables in part
    order, saturated to +-65504 and rounded to f16 (pure additions: exact here).  partial: (entries, 2) float32 as the record's
    `partial` addresses it.  Returns the (2 * offsets[-1]) values as float16."""
    partial = np.asarray(partial, f32).reshape(-1, 2)
    out = np.zeros((offsets[-1], 2), f32)
    for l in range(len(k_split)):
        size = offsets[l + 1] - offsets[l]
        acc = np.zeros((size, 2), f32)
        for k in range(k_split[l]):
            acc = acc + partial[part_off[l] + k * size: part_off[l] + (k + 1) * size]
        out[offsets[l]:offsets[l + 1]] = acc
    return np.clip(out, f32(-F16_MAX), f32(F16_MAX)).astype(np.float16).reshape(-1)


def bias_correction_deviation(beta, steps):
    """float32 bias corrections fl32(1 - fl32(beta^t)) against apex's (1 - beta**t in double, rounded to float32), beta being
    the float32 the launcher receives: returns per step (|difference|, ulp32(beta^t), ulp32(bc), bc), absolute."""
    t = np.asarray(steps, f64)
    pw = np.power(f32(beta), t.astype(f32), dtype=f32)
    bc32 = (f32(1) - pw).astype(f64)
    bc64 = (1.0 - np.power(float(f32(beta)), t)).astype(f32).astype(f64)
    return np.abs(bc32 - bc64), ulp32(pw), ulp32(bc64), bc64


# ------------------------------------------------------------------------------------------------------------------------------
# loss seeds, terms and blend
# ------------------------------------------------------------------------------------------------------------------------------

# Absolute error of the device logarithm, in units of E max(1, |log x|), over LOG_SWEEP (the opacities the tests use), measured
# once on an MI355X against the float64 logarithm as the issue prescribes (test_device_logarithms_stay_inside_tau repeats the
# measurement on every run and prints it):
#   __logf (through ngp_nerf_loss, d_o = -(lg + 1) / 256):          measured 2.925   -> 4 x = 11.7  -> TAU_FAST = 16
#   logf   (through ngp_nerf_loss_terms_fw, ent = -(o log o)):       measured 2.862   -> 4 x = 11.4  -> TAU_LOGF = 16
# (both figures include the one rounded operation through which the logarithm is observed, up to 1 unit; one float32 ulp of a
# logarithm is up to 2 units).  The tolerance is 4 x the measured maximum, rounded up to a power of two (room for another
# compiler version's expansion).  A MEASURED value above 16 = 2^-20 / E would be a defect, not a tolerance.
MEASURED_TAU_FAST = 2.925
MEASURED_TAU_LOGF = 2.862
TAU_FAST = 16.0
TAU_LOGF = 16.0
TAU_DEFECT = 16.0
LOSS_EPS = f32(1e-10)


def log_sweep():
    """The opacities of the loss tests: 0, 1e-10 .. 1e-3 by decades, 4096 values in [0.9, 1], exactly 1, and 1024 values across
    [1e-3, 0.9] so that the middle of the range is not left out."""
    return np.concatenate([[0.0], 10.0 ** np.arange(-10, -2), np.linspace(0.9, 1.0, 4096), [1.0],
                           np.linspace(1e-3, 0.9, 1024)]).astype(f32)


def tau_units(lg_device, oe):
    """|lg_device - log(oe)| in units of E max(1, |log oe|)."""
    ref = np.log(np.asarray(oe, f64))
    return np.abs(np.asarray(lg_device, f64) - ref) / (E * np.maximum(1.0, np.abs(ref)))


def _log_oe(opacity):
    """fl32(o + 1e-10f) (one float32 operation, formed first), its float64 logarithm, and the scale max(1, |log|) of tau."""
    oe = (np.asarray(opacity, f32) + LOSS_EPS).astype(f64)
    lg = np.log(oe)
    return oe, lg, np.maximum(1.0, np.abs(lg))


def nerf_loss_ref(rgb, opacity, gt, bg, lambda_o, grad_scale, tau=None):
    """ngp_pl_amd.losses.mean_loss_and_seeds in float64 (1 / n and 1 / (3 n) exact), and per-ray bounds that follow nerf_loss_ray
    (loss_common.h; contraction is off there) operation by operation.  tau: the device logarithm's error in units of
    E max(1, |log|) (TAU_FAST by default).

    Returns dict: loss, sq_err (float64 scalars), d_rgb (R,3), d_o (R), their bounds e_d_rgb, e_d_o, and what the reductions need:
    l_ray, se_ray (per-ray terms of loss / sq_err), e_l, e_se (sum over rays of the per-ray term errors).

    With b = bg[k] (0 without a background), inv_3r = fl32(1 / fl32(3 n)) and inv_r = fl32(1 / n) carry one rounding each (3 n is
    exact below 2^24):
        t1 = 1 - o;  t2 = b t1;  t3 = c + t2;  diff = t3 - g     e_diff = E (2 |t2| + |t3| + |diff|)    (b = 0: t3 = c exactly)
        se_ray = sum diff^2                                       e_se = sum (2 |diff| e_diff + E diff^2) + 2 E se_ray
        gr = (2 diff) inv_3r                                      e_gr = 2 e_diff / (3 n) + 3 E |gr|      (inv_3r, product; + 1)
        d_rgb = gr grad_scale                                     e = grad_scale e_gr + E |d_rgb|
        x_k = gr b                                                e_x = |b| e_gr + E |x_k|
        lg = log(oe) +- tau E max(1, |log oe|)
        w = lambda (-(lg + 1)) inv_r                              e_w = lambda e_lg / n + 4 E |w|  (sum, product, inv_r, product)
        go = -x_0 - x_1 - x_2 + w                                 three roundings of partial sums: 3 -> 4 E (sum |x_k| + |w|)
        d_o = go grad_scale                                       e = grad_scale (sum e_x + e_w + 4 E (...)) + E |d_o|
        h = lambda (-oe lg) inv_r                                 e_h = lambda oe e_lg / n + 4 E |h|
        l_ray = se_ray inv_3r + h                                 e = e_se / (3 n) + 3 E se_ray / (3 n) + e_h + E |l_ray|"""
    tau = TAU_FAST if tau is None else tau
    rgb, gt = np.asarray(rgb, f64).reshape(-1, 3), np.asarray(gt, f64).reshape(-1, 3)
    o = np.asarray(opacity, f64)
    n = o.shape[0]
    lam, gs = float(f32(lambda_o)), float(f32(grad_scale))
    b = np.zeros(3) if bg is None else np.asarray(bg, f64)
    t1 = (1.0 - o)[:, None]
    t2 = b[None, :] * t1
    t3 = rgb + t2
    diff = t3 - gt
    e_diff = E * np.abs(diff) if bg is None else E * (2 * np.abs(t2) + np.abs(t3) + np.abs(diff))
    se_ray = (diff * diff).sum(1)
    e_se = (2 * np.abs(diff) * e_diff + E * diff * diff).sum(1) + 2 * E * se_ray
    gr = 2.0 * diff / (3 * n)
    e_gr = 2 * e_diff / (3 * n) + 3 * E * np.abs(gr)
    d_rgb = gr * gs
    e_d_rgb = gs * e_gr + E * np.abs(d_rgb) + TINY
    x = gr * b[None, :]
    e_x = np.abs(b)[None, :] * e_gr + E * np.abs(x)
    oe, lg, lscale = _log_oe(opacity)
    e_lg = tau * E * lscale
    w = lam * (-(lg + 1.0)) / n
    e_w = lam * e_lg / n + 4 * E * np.abs(w)
    go = -x.sum(1) + w
    mag = np.abs(x).sum(1) + np.abs(w)
    d_o = go * gs
    e_d_o = gs * (e_x.sum(1) + e_w + 4 * E * mag) + E * np.abs(d_o) + TINY
    h = lam * (-oe * lg) / n
    e_h = lam * oe * e_lg / n + 4 * E * np.abs(h)
    a = se_ray / (3 * n)
    l_ray = a + h
    e_l = e_se / (3 * n) + 3 * E * a + e_h + E * np.abs(l_ray) + TINY
    return dict(loss=l_ray.sum(), sq_err=se_ray.sum(), d_rgb=d_rgb, d_o=d_o, e_d_rgb=e_d_rgb, e_d_o=e_d_o,
                l_ray=l_ray, se_ray=se_ray, e_l=e_l.sum(), e_se=e_se.sum())


def loss_workgroups(n_rays):
    return -(-n_rays // 256)


def loss_reduction_k(n_rays):
    """Additions a per-ray term passes through in nerf_loss_kernel.  Overwrite mode (n_rays <= 16384): 6 levels of the wave sum,
    2 to combine the four waves, 6 levels of the wave sum over the workgroups' partials: 14.  Atomic mode: 6 + 2 and then at
    most one atomic addition per workgroup: 8 + workgroups."""
    return 14 if n_rays <= 16384 else 8 + loss_workgroups(n_rays)


def wave_sum_f32(v):
    """ngp_wave_sum (ngp_common.h) of 64 float32 lanes: the butterfly v += shfl_xor(v, 32), 16, .. 1, in float32."""
    v = np.asarray(v, f32)
    assert v.shape[0] == 64
    for half in (32, 16, 8, 4, 2, 1):
        v = v[:half] + v[half:2 * half]
    return v[0]


def overwrite_sum_f32(per_ray):
    """nerf_loss_kernel<OVERWRITE>'s reduction of float32 per-ray terms, bit for bit: per workgroup of 256 rays the wave sums of
    its four waves combined (s0 + s1) + (s2 + s3), then one wave sum over the workgroups' partials in workgroup order."""
    per_ray = np.asarray(per_ray, f32)
    blocks = loss_workgroups(per_ray.shape[0])
    assert blocks <= 64
    pad = np.zeros(blocks * 256, f32)
    pad[:per_ray.shape[0]] = per_ray
    parts = np.zeros(64, f32)
    for blk in range(blocks):
        s = [wave_sum_f32(pad[blk * 256 + w * 64: blk * 256 + (w + 1) * 64]) for w in range(4)]
        parts[blk] = (s[0] + s[1]) + (s[2] + s[3])
    return wave_sum_f32(parts), parts[:blocks]


def loss_terms_ref(rgb, opacity, gt, lambda_o, tau=None):
    """ngp_nerf_loss_terms_fw: sq (R,3) = (rgb - gt)^2, ent (R) = lambda (-(oe log oe)), in float64 with bounds.
        d = rgb - gt; sq = d d        e_sq = 3 E sq                      (d's rounding twice, the product)
        ent                           e_ent = lambda oe e_lg + 3 E |ent|  (two products: 2 -> 3)"""
    tau = TAU_LOGF if tau is None else tau
    d = np.asarray(rgb, f64).reshape(-1, 3) - np.asarray(gt, f64).reshape(-1, 3)
    lam = float(f32(lambda_o))
    oe, lg, lscale = _log_oe(opacity)
    sq = d * d
    ent = lam * (-oe * lg)
    return dict(sq=sq, e_sq=3 * E * sq + TINY, ent=ent, e_ent=lam * oe * tau * E * lscale + 3 * E * np.abs(ent) + TINY)


def loss_terms_bw_ref(g_sq, g_ent, rgb, opacity, gt, lambda_o, tau=None):
    """ngp_nerf_loss_terms_bw: g_rgb = g_sq (2 (rgb - gt)), g_opacity = g_ent (lambda (-(log oe + 1))).  g_sq (R,3) or scalar,
    g_ent (R) or scalar.
        g_rgb      the difference, the product (doubling is exact): 2 -> 3 E |g_rgb|
        g_opacity  e = |g_ent| lambda e_lg + 4 E |g_opacity|   (sum, two products: 3 -> 4)"""
    tau = TAU_LOGF if tau is None else tau
    d = np.asarray(rgb, f64).reshape(-1, 3) - np.asarray(gt, f64).reshape(-1, 3)
    lam = float(f32(lambda_o))
    g_sq = np.broadcast_to(np.asarray(g_sq, f64), d.shape) if np.ndim(g_sq) == 0 else np.asarray(g_sq, f64).reshape(-1, 3)
    _, lg, lscale = _log_oe(opacity)
    g_ent = np.broadcast_to(np.asarray(g_ent, f64), lg.shape)
    g_rgb = g_sq * (2.0 * d)
    g_op = g_ent * (lam * (-(lg + 1.0)))
    return dict(g_rgb=g_rgb, e_g_rgb=3 * E * np.abs(g_rgb) + TINY, g_opacity=g_op,
                e_g_opacity=np.abs(g_ent) * lam * tau * E * lscale + 4 * E * np.abs(g_op) + TINY)


def bg_blend_ref(rgb, opacity, bg):
    """ngp_bg_blend: fma(bg, fl32(1 - o), rgb) in float64 (fl32(1 - o) formed in float32 first: one operation); the result of a
    fused multiply-add is the correctly rounded value, so the device is within one float32 ulp of it (half an ulp, were the
    float64 evaluation exact)."""
    tr = (f32(1) - np.asarray(opacity, f32)).astype(f64)
    return np.asarray(rgb, f64).reshape(-1, 3) + np.asarray(bg, f64)[None, :] * tr[:, None]


def bg_blend_bw_ref(g_rgb, g_opacity, bg):
    """ngp_bg_blend_bw: g_opacity (0 if None) - sum_c g_rgb[., c] bg[c]; three fused multiply-adds, one rounding each on a partial
    sum no larger than the sum of the terms' magnitudes: 3 E sum |terms|."""
    g_rgb = np.asarray(g_rgb, f64).reshape(-1, 3)
    g0 = np.zeros(g_rgb.shape[0]) if g_opacity is None else np.asarray(g_opacity, f64)
    terms = g_rgb * np.asarray(bg, f64)[None, :]
    return g0 - terms.sum(1), 3 * E * (np.abs(g0) + np.abs(terms).sum(1)) + TINY


# ------------------------------------------------------------------------------------------------------------------------------
# AMP plumbing (exact)
# ------------------------------------------------------------------------------------------------------------------------------

def cast_inputs():
    """float32 inputs of the f32 -> f16 cast test: for every finite f16 value h its float32 image, that image's two float32
    neighbours, the midpoint between h and the next f16 value away from zero (the tie; beyond 65504 that is 65520, which rounds
    to inf) and the midpoint's two neighbours; +-inf, values beyond 65520, the f16 subnormal boundaries, float32 subnormals and
    +-0."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    h = bits.view(np.float16)
    h = h[np.isfinite(h)]
    x = h.astype(f32)
    away = np.where(np.signbit(x), f32(-np.inf), f32(np.inf)).astype(f32)
    step = np.where(np.abs(x) < 2.0 ** -14, 2.0 ** -24, ulp32(x) * 2.0 ** 13)          # f16 spacing at |h|
    mid = (x.astype(f64) + np.where(np.signbit(x), -0.5, 0.5) * step).astype(f32)       # exact in float32
    parts = [x, np.nextafter(x, away), np.nextafter(x, -away), mid, np.nextafter(mid, away), np.nextafter(mid, -away)]
    extra = []
    for s in (1.0, -1.0):
        extra += [s * np.inf, s * 65519.996, s * 65520.0, s * 65520.004, s * 65536.0, s * 1e5, s * 3.4028234663852886e38,
                  s * 2.0 ** -14, s * 2.0 ** -24, s * 2.0 ** -25, s * 1.0000001 * 2.0 ** -25, s * 0.9999999 * 2.0 ** -25,
                  s * 1.5 * 2.0 ** -24, s * 2.0 ** -26, s * 2.0 ** -126, s * 2.0 ** -149, s * 0.0]
    return np.concatenate(parts + [np.asarray(extra, f32)]).astype(f32)


def sum_slices_ref(own, stage, rank):
    """ngp_sum_slices_f16: float32 sum over the world slices in rank order (slice `rank` is `own`, stage[rank] is ignored), one
    rounding to f16; no saturation (a sum beyond the f16 range is inf)."""
    stage = np.asarray(stage, np.float16)
    acc = np.zeros(stage.shape[1], f32)
    for q in range(stage.shape[0]):
        acc = acc + (np.asarray(own, np.float16) if q == rank else stage[q]).astype(f32)
    with np.errstate(over="ignore"):
        return acc.astype(np.float16)


# ------------------------------------------------------------------------------------------------------------------------------
# the cases, shared by the CPU proof of the bounds and the GPU test
# ------------------------------------------------------------------------------------------------------------------------------

ADAM_SIZES = (1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1027)
ADAM_LARGE = 4_194_304 + 7                  # above 4096 * 256 * 4: the grid-stride loop takes a second trip
ADAM_STEPS = (1, 2, 1000, 30000)
ADAM_WDS = (0.0, 1e-2)
ADAM_SCALES = (1.0, 128.0, 3.0)             # 3 is no power of two: inv_scale is rounded
PARTIALS_ROWS = (0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 37, 256)
PARTIALS_N = (1, 31, 32, 33, 3072)
REDUCE_ROWS = (0, 1, 7, 8, 9, 24, 25, 31, 32, 33, 57, 256)
REDUCE_NA = (1, 31, 32, 33)
REDUCE_NB = (0, 1, 33)

# special elements planted among the random ones (adam_dense_inputs): name -> (m, v, raw gradient); None keeps the random value
_INF, _NAN = float("inf"), float("nan")
SPECIALS = (("zero", 0.0, 0.0, 0.0),                  # g = m = v = 0: with wd = 0 the parameter must not change by a bit
            ("subnormal_m", 1.2e-38, 1e-12, 0.0),     # m is normal, beta1 m is subnormal
            ("eps_path", 1e-3, 0.0, 0.0),             # v' = 0: the denominator is eps alone
            ("g_max", None, None, F16_MAX), ("g_min", None, None, -F16_MAX),
            ("g_inf", None, None, _INF), ("g_ninf", None, None, -_INF), ("g_nan", None, None, _NAN))
_F32_LARGE = (F16_MAX, -F16_MAX, 3.0e4, -1.2345678e4, 1.0e4)      # the f32 path is unclamped: finite values instead


def adam_dense_inputs(n, grad_is_f32, grad_scale, seed=0):
    """(p, m, v float32; g float16 or float32; kind (n) int: index into SPECIALS or -1).  Magnitudes spread over decades, signs
    mixed, non-zero moments; every third element (offset by n, so that the sizes put different specials into the vector body and
    the scalar tail) is a special."""
    rng = np.random.default_rng(1000 * seed + n)
    sign = lambda: rng.choice([-1.0, 1.0], n)
    p = (sign() * 10.0 ** rng.uniform(-4, 1, n)).astype(f32)
    m = (sign() * 10.0 ** rng.uniform(-8, -1, n)).astype(f32)
    v = (10.0 ** rng.uniform(-14, -2, n)).astype(f32)
    g = sign() * 10.0 ** rng.uniform(-6, 2, n) * grad_scale
    idx = np.arange(n)
    idx = idx[(idx + n) % 3 == 0]
    kind = np.full(n, -1)
    kind[idx] = ((idx + n) // 3) % len(SPECIALS)
    for k, (_, sm, sv, sg) in enumerate(SPECIALS):
        at = kind == k
        if sm is not None:
            m[at], v[at] = sm, sv
        g[at] = sg if not (grad_is_f32 and k >= 3) else _F32_LARGE[k - 3]
    with np.errstate(over="ignore"):
        g = g.astype(f32) if grad_is_f32 else g.astype(np.float16)
    return p, m, v, g, kind


def adam_dense_reference(p, m, v, g, coef):
    """Reference and bounds of one dense step.  f16 gradients are clamped (clamp_f16_grad); returns a list of one or two
    ((p', m', v'), (e_p, e_m, e_v), applies) alternatives: the second differs where the gradient is NaN (-65504 for +65504)."""
    if g.dtype == np.float16:
        gc, nan = clamp_f16_grad(g)
        alts = [adam_ref(p, m, v, gc, coef)]
        if nan.any():
            alts.append(adam_ref(p, m, v, np.where(nan, -F16_MAX, gc), coef))
        return alts
    return [adam_ref(p, m, v, g.astype(f64), coef)]


def worst_fraction(got, alts):
    """max over elements of |got - ref| / bound for (p, m, v), an element taking the alternative that suits all three best.
    got: (p, m, v) arrays.  Returns three floats."""
    fr = []
    for ref, err in alts:
        fr.append(np.stack([np.abs(np.asarray(x, f64) - r) / e for x, r, e in zip(got, ref, err)]))      # (3, n)
    fr = np.stack(fr)                                                                                   # (alts, 3, n)
    pick = np.argmin(fr.max(1), axis=0)                                                                 # per element
    best = np.take_along_axis(fr, pick[None, None, :], 0)[0]
    best = np.where(np.isnan(best), np.inf, best)
    return tuple(float(best[k].max()) if best.shape[1] else 0.0 for k in range(3))


def adam_combos():
    """Every (step, weight decay, grad scale) of the dense cases."""
    return [(t, wd, gs) for t in ADAM_STEPS for wd in ADAM_WDS for gs in ADAM_SCALES]


def partials_inputs(n_partials, n, seed=0):
    """(p, m, v float32 (n); rows float32 (n_partials, n)): rows of mixed sign and magnitude (1e-2 .. 1e1), so that a dropped or
    repeated row moves the sum by orders of magnitude more than the summation bound; v >= 1e-6 keeps the update well conditioned
    where a column sum cancels."""
    rng = np.random.default_rng(77 + 1000 * seed + 7919 * n_partials + n)
    sign = lambda shape: rng.choice([-1.0, 1.0], shape)
    p = (sign(n) * 10.0 ** rng.uniform(-3, 0, n)).astype(f32)
    m = (sign(n) * 10.0 ** rng.uniform(-5, -1, n)).astype(f32)
    v = (10.0 ** rng.uniform(-6, -2, n)).astype(f32)
    rows = (sign((n_partials, n)) * 10.0 ** rng.uniform(-2, 1, (n_partials, n))).astype(f32)
    return p, m, v, rows


def partials_combo(n_partials, n):
    """The (step, weight decay, grad scale) a partials case runs with: cycles through all of them across the cases."""
    c = adam_combos()
    return c[(PARTIALS_ROWS.index(n_partials) * len(PARTIALS_N) + PARTIALS_N.index(n)) % len(c)]


def adam_partials_reference(p, m, v, rows, coef, extra=9):
    """Reference of adam_from_partials: the float64 column sum as the raw gradient, its float32 summation bound propagated."""
    rows64 = np.asarray(rows, f64)
    g = rows64.sum(0) if rows64.shape[0] else np.zeros(rows64.shape[1])
    e = reduce_bound(rows64, extra) if rows64.shape[0] else np.zeros(rows64.shape[1])
    return adam_ref(p, m, v, g, coef, e)


def adam_partials_f32(p, m, v, rows, coef):
    """adam_from_partials in uncontracted numpy float32, with its summation order (two accumulators per row lane, 16-row stride,
    8-row tail, the 8 lanes added in order)."""
    rows = np.asarray(rows, f32)
    n_partials, n = rows.shape
    lanes = np.zeros((8, n), f32)
    for r in range(8):
        a0, a1 = np.zeros(n, f32), np.zeros(n, f32)
        q = r
        while q + 8 < n_partials:
            a0 = a0 + rows[q]; a1 = a1 + rows[q + 8]
            q += 16
        while q < n_partials:
            a0 = a0 + rows[q]
            q += 8
        lanes[r] = a0 + a1
    g = np.zeros(n, f32)
    for r in range(8):
        g = g + lanes[r]
    return adam_f32(p, m, v, g, coef)
