"""TEST INFRASTRUCTURE -- the hash-grid forward and its input gradient, restated in plain numpy from the CONTRACT of csrc/hashgrid.hip /
csrc/hashgrid_common.h: no waves, chunks, cell runs, lists or XCD maps in here.  The cell arithmetic is the one of
tests/table_backward_reference.py (fma_f32, unit_positions, corner_indices, corner_weights), imported, not copied.

Per (sample, level):

  x01   = f32((x - min) * inv), inv = 1 / (max - min)                    [load_box, cell_of]
  pos   = fmaf(x01, scale, 0.5);  fl = floor(pos);  f = pos - fl  (exact);  cell = (uint32)(int)fl, wrapped into 32 bits
  idx   = corner_indices<hashed>(cell)      hashed iff res^3 > size.  OUTSIDE the box the kernel's semantics are kept: on a dense level
          every coordinate is clamped with min((uint32)cell, res - 1) -- a cell above res - 1 AND a negative cell (a huge unsigned
          value) both land on the border cell res - 1 -- and on a hashed level the wrapped 32-bit cell is hashed as it is.  The weights
          are left as computed from f in either case.
  exact = sum_c W_c * v_c,  mass = sum_c |W_c| * |v_c|     in float64; W_c = the product of the three factors f_k or 1 - f_k taken from
          the f32 f above, v_c = the f16 table entry at the corner
  emulated = the kernel's own operation order: w_c = corner_weights (f32, ((wx * wy) * wz)), o = fmaf(w_c, f32(v_c), o) for c = 0 .. 7
          from o = 0, then ONE conversion of o to f16, round to nearest even.

LIMIT per output, derived, not measured (u = 2^-24, gamma_k = k u / (1 - k u)):

  |out - exact| <= gamma_11 * mass + 1/2 * ulp16(|exact| + gamma_11 * mass)

A term w_c * v_c passes through at most 3 roundings in its weight (1 - f, two products) and at most 8 fmafs, 11 factors (1 + d),
|d| <= u, hence |o - exact| <= gamma_11 * mass (Higham, Accuracy and Stability, lemma 3.1); the conversion to f16 adds half a spacing
of f16 at |o| <= |exact| + gamma_11 * mass (ulp16 is floored at 2^-24: subnormal outputs).  The relative model needs every f32
result to be zero or normal: inside the box f and 1 - f are zero or at least 2^-24, a weight at least 2^-72, a term at least 2^-96;
forward_level() refuses inputs whose weights fall below 2^-100 instead of holding them to a bound that does not cover them.  The
float64 evaluation of exact and mass itself is off by less than 2^-49 * mass, four million times below gamma_11 * mass, and inside the box
1 - f is exact in f32 (2 roundings per weight, not 3), which leaves that room.

The same for ngp_hashgrid_bwd_input (input_gradient_reference): per sample and axis k, from the kernel's cell,

  grad_k = out_scale * sum_l scale_l * inv_k * sum_c w'_c * (t0 d0 + t1 d1)                                 in float64
  mass_k = |out_scale| * sum_l scale_l * inv_k * sum_c |w'_c| * (|t0 d0| + |t1 d1|)
  |out_k - grad_k| <= gamma_32 * mass_k

w'_c = +-1 along k times the other two factors; (t0, t1) the corner's table entry, (d0, d1) the level's upstream gradient.  32 roundings
at most on the way of any term: 3 for the corner's value t0 d0 + t1 d1, 3 for its weight, 8 for the corner sum, 1 for scale * inv, 16
level fmafs, 1 for out_scale.  That file is compiled with contraction allowed: roundings are counted, no order is pinned, and there is
no emulation of this kernel.

LIMITS OF THIS RESTATEMENT: box extents must be powers of two (unit_positions refuses others: v_rcp_f32 is 1 ulp off there), and
|pos| must stay below 2^31 (the kernel's float -> int conversion is only defined there)."""
from types import SimpleNamespace

import numpy as np

from tests import table_backward_reference as R

U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


def fma_f32(a, b, c):
    """fmaf(a, b, c) for f32 arrays and ANY f32 addend c whose result is zero or a normal f32: the exact a * b + c rounded once.

    R.fma_f32 argues its case for c = 0.5; the argument for a general c.  p = a * b is exact in f64 (48 bits).  s = fl64(p + c) and
    TwoSum's err satisfy s + err == p + c exactly, with |err| <= half an f64 spacing at s.  Every midpoint m of two neighbouring normal
    f32 is an f64 (25 significant bits) and rounding to f64 is monotone, so p + c < m implies s <= m and p + c > m implies s >= m:
      * s is not a midpoint: s lies strictly on the same side of every midpoint as p + c, and f32(s) = f32(p + c);
      * s is a midpoint: err == 0 means p + c is that midpoint and ties-to-even of s is the fma's rounding; err != 0 means p + c lies
        strictly on err's side of it, and moving s one f64 step that way puts it strictly between the midpoint and the f32 neighbour,
        so f32() rounds to the neighbour the fma picks.
    That is what R.fma_f32 computes; what it does not cover are f32 SUBNORMAL results, whose midpoints sit at other bits: refused."""
    out = R.fma_f32(np.asarray(a, np.float32), np.asarray(b, np.float32), c)
    if ((out != 0) & (np.abs(out) < np.float32(2.0 ** -126))).any():
        raise ValueError("fma_f32: a subnormal f32 result, outside what the midpoint test covers")
    return out


def cell_from_pos(pos):
    """pos (n, 3) f32 -> cell (n, 3) uint32 = (uint32)(int)floorf(pos), f (n, 3) f32 = pos - floorf(pos) (exact)."""
    if not (np.abs(pos) < 2.0 ** 31).all():
        raise ValueError("|pos| must stay below 2^31")
    fl = np.floor(pos)
    return fl.astype(np.int64).astype(np.uint32), (pos - fl).astype(np.float32)


def cells_of(x, xyz_min, xyz_max, scale):
    """The kernel's own cell, bit for bit.  Returns pos, cell, f."""
    x01 = R.unit_positions(x, xyz_min, xyz_max)
    pos = R.fma_f32(x01, np.full((1, 1), scale, np.float32), 0.5)
    return (pos,) + cell_from_pos(pos)


def exact_weights(f):
    """f (n, 3) f32 -> (8, n) f64 products of f_k or 1 - f_k, every factor exact."""
    f = f.astype(np.float64)
    out = np.empty((8, f.shape[0]))
    for c in range(8):
        out[c] = ((f[:, 0] if c & 1 else 1 - f[:, 0]) * (f[:, 1] if (c >> 1) & 1 else 1 - f[:, 1])) * (f[:, 2] if c >> 2 else 1 - f[:, 2])
    return out


def emulate(f, v):
    """f (n, 3) f32, v (8, n, 2) f16 corner values -> (n, 2) f16 in the kernel's operation order."""
    w = R.corner_weights(f)
    o = np.zeros(v.shape[1:], np.float32)
    for c in range(8):
        o = fma_f32(np.broadcast_to(w[c][:, None], o.shape), v[c].astype(np.float32), o)
    return o.astype(np.float16)


def limit(exact, mass, k=11):
    return gamma(k) * mass + 0.5 * R.ulp16(np.abs(exact) + gamma(k) * mass)


def forward_level(x, xyz_min, xyz_max, table, res, offset, size, scale):
    """One level: cell, f, idx (8, n) inside the level, exact / mass / limit (n, 2) f64, emulated (n, 2) f16."""
    assert table.dtype == np.float16 and table.ndim == 2 and table.shape[1] == 2
    pos, cell, f = cells_of(x, xyz_min, xyz_max, scale)
    hashed = R.is_hashed(res, size)
    idx = R.corner_indices(cell, res, size, hashed)
    assert idx.min(initial=0) >= 0 and idx.max(initial=0) < size
    v = table[offset + idx]                                          # (8, n, 2) f16
    W = exact_weights(f)
    if ((W != 0) & (W < 2.0 ** -100)).any():
        raise ValueError("a corner weight below 2^-100: f32 underflow is outside the relative-error model of the limit")
    v64 = v.astype(np.float64)
    exact = (W[:, :, None] * v64).sum(axis=0)
    mass = (W[:, :, None] * np.abs(v64)).sum(axis=0)
    return SimpleNamespace(pos=pos, cell=cell, f=f, idx=idx, v=v, hashed=hashed, res=res, size=size, offset=offset, scale=scale,
                           exact=exact, mass=mass, limit=limit(exact, mass), emulated=emulate(f, v))


def forward_reference(x, xyz_min, xyz_max, table, resolution, offset, scale, n_levels):
    """x (n, 3) f32, table (total, 2) f16.  Returns exact / mass / limit (L, n, 2) f64, emulated (L, n, 2) f16, levels."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 3)
    lv = [forward_level(x, xyz_min, xyz_max, table, int(resolution[l]), int(offset[l]), int(offset[l + 1]) - int(offset[l]), scale[l])
          for l in range(n_levels)]
    stack = lambda name: np.stack([getattr(v, name) for v in lv]) if lv else None
    return SimpleNamespace(n=x.shape[0], n_levels=n_levels, levels=lv, exact=stack("exact"), mass=stack("mass"), limit=stack("limit"),
                           emulated=stack("emulated"))


def out_of_limit(got, ref, rows=None):
    """got (L, m, 2) f16 against ref (rows: the samples of ref that got's columns are).  Returns (the number of outputs beyond their
    limit or not finite, a description of the worst, the worst error / limit)."""
    exact, lim = (ref.exact, ref.limit) if rows is None else (ref.exact[:, rows], ref.limit[:, rows])
    g = got.astype(np.float64)
    assert g.shape == exact.shape, (g.shape, exact.shape)
    if g.size == 0:
        return 0, "", 0.0
    with np.errstate(invalid="ignore"):
        err = np.abs(g - exact)
        ratio = np.where(np.isfinite(g), err / lim, np.inf)
    bad = ~(ratio <= 1.0)
    l, i, k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    what = "worst error/limit %.4f at level %d sample %d feature %d: got %r, exact %r, limit %.3g" % (
        float(ratio[l, i, k]), l, i, k, float(g[l, i, k]), float(exact[l, i, k]), float(lim[l, i, k]))
    return int(bad.sum()), what, float(ratio.max())


def share_equal(got, ref, rows=None):
    """Share of outputs whose 16 bits equal the emulation's (the sign of a zero counts)."""
    emu = ref.emulated if rows is None else ref.emulated[:, rows]
    return float((got.view(np.int16) == emu.view(np.int16)).mean()) if emu.size else 1.0


def input_gradient_reference(x, xyz_min, xyz_max, table, dfeats, resolution, offset, scale, n_levels, out_scale):
    """dfeats (L, n, 2) f16 -> grad (n, 3) f64, mass (n, 3) f64, limit = gamma_32 * mass."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 3)
    assert dfeats.dtype == np.float16 and dfeats.shape == (n_levels, x.shape[0], 2)
    ext = np.asarray(xyz_max, np.float32).reshape(3) - np.asarray(xyz_min, np.float32).reshape(3)
    inv = (np.float32(1.0) / ext).astype(np.float64)                  # exact: unit_positions insists on powers of two
    grad = np.zeros((x.shape[0], 3))
    mass = np.zeros((x.shape[0], 3))
    for l in range(n_levels):
        res, off, size = int(resolution[l]), int(offset[l]), int(offset[l + 1]) - int(offset[l])
        _, cell, f = cells_of(x, xyz_min, xyz_max, scale[l])
        idx = R.corner_indices(cell, res, size, R.is_hashed(res, size))
        t = table[off + idx].astype(np.float64)                       # (8, n, 2)
        d = dfeats[l].astype(np.float64)[None]                        # (1, n, 2)
        val = (t * d).sum(axis=2)
        aval = np.abs(t * d).sum(axis=2)
        f64 = f.astype(np.float64)
        s = np.float64(np.float32(scale[l]))
        for k in range(3):
            a, b = [j for j in range(3) if j != k]
            acc = np.zeros(x.shape[0])
            am = np.zeros(x.shape[0])
            for c in range(8):
                w = (f64[:, a] if (c >> a) & 1 else 1 - f64[:, a]) * (f64[:, b] if (c >> b) & 1 else 1 - f64[:, b])
                acc += (w if (c >> k) & 1 else -w) * val[c]
                am += w * aval[c]
            grad[:, k] += s * inv[k] * acc
            mass[:, k] += s * inv[k] * am
    return SimpleNamespace(grad=grad * out_scale, mass=mass * abs(out_scale), limit=gamma(32) * mass * abs(out_scale))
