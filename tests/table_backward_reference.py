"""TEST INFRASTRUCTURE -- the table backward of the hash grid as exact integers, in plain numpy.

Restated from the CONTRACT of csrc/hashgrid_bwd_binned.hip / csrc/hashgrid_common.h, not from the kernel's loops: there are no
chunks, slices, task orders or splits in here.  Per (sample, level):

  x01  = f32((x - min) * inv), inv = 1 / (max - min)                     [load_box, cell_of_loaded]
  pos  = fmaf(x01, scale, 0.5); cell = floor(pos); f = pos - cell
  idx  = corner_indices<hashed>(cell)        hashed iff res^3 > size
  w    = ((cx ? fx : 1 - fx) * (cy ? fy : 1 - fy)) * (cz ? fz : 1 - fz)   in f32, this association      [corner_weight]
  q    = rint(f64(f32(w * f32(g))) * 2^24)   ties to even, one 64-bit integer per corner and feature   [fix_q64]
  Q[idx] += q                                integer adds: no order can change a bit

and the write-out  f16(clip(f32(Q) * 2^-24, +-65504)),  both conversions round to nearest even.

LIMIT: box extents must be powers of two.  The kernel takes 1 / (max - min) from v_rcp_f32, which is exact for a power of two and
up to 1 ulp off for anything else; this restatement divides, and refuses every other extent rather than disagreeing about it.
Points are expected inside the closed box (outside it the kernel's cell is "arbitrary but in bounds").
"""
from types import SimpleNamespace

import numpy as np

PRIME_Y, PRIME_Z = 2654435761, 805459861
FIX_ONE = float(1 << 24)                    # fixed-point units per 1.0
F16_MAX = 65504.0
_M32 = np.uint64(0xFFFFFFFF)


def fma_f32(a, b, c):
    """fmaf(a, b, c) for f32 arrays: the exact a*b + c, rounded ONCE to f32.

    The f64 product of two f32 is exact (48 bits).  For the magnitudes here (a*b is 0 or at least half a cell, below 2^16) the
    f64 sum with 0.5 is exact as well (at most 49 bits), so the rounding to f32 is the only one: the fma's.  Where a*b is a tiny
    non-zero number the sum can need more than 53 bits; TwoSum recovers what the f64 add dropped, and it matters only when the f64
    sum sits exactly on the midpoint of two f32 neighbours: there the dropped part decides the direction, as it does in the fma."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                                  # exact: s + err == p + c
    tie = (s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    nudge = tie & (err != 0)
    if nudge.any():
        s = s.copy()
        s[nudge] = np.nextafter(s[nudge], np.where(err[nudge] > 0, np.inf, -np.inf))
    return s.astype(np.float32)


def is_hashed(res, size):
    return int(res) ** 3 > int(size)


def corner_indices(cell, res, size, hashed):
    """cell (m, 3) uint32 -> (8, m) int64 indices inside the level; corner c = cx + 2 cy + 4 cz."""
    c64 = cell.astype(np.uint64)
    out = np.empty((8, cell.shape[0]), np.int64)
    if hashed:
        assert size & (size - 1) == 0, "hashed levels have a power-of-two size (the index is masked)"
        for c in range(8):
            hx = (c64[:, 0] + np.uint64(c & 1)) & _M32
            hy = ((c64[:, 1] + np.uint64((c >> 1) & 1)) * np.uint64(PRIME_Y)) & _M32
            hz = ((c64[:, 2] + np.uint64(c >> 2)) * np.uint64(PRIME_Z)) & _M32
            out[c] = ((hx ^ hy ^ hz) & np.uint64(size - 1)).astype(np.int64)
    else:
        top = np.uint64(res - 1)                                     # border clamp: a no-op for points inside the box
        base = np.minimum(c64[:, 0], top) + np.minimum(c64[:, 1], top) * np.uint64(res) + np.minimum(c64[:, 2], top) * np.uint64(res * res)
        for c in range(8):
            i = (base + np.uint64((c & 1) + ((c >> 1) & 1) * res + (c >> 2) * res * res)).astype(np.int64)
            out[c] = np.where(i >= size, i - size, i)                # one conditional subtract, as the kernel has it
    return out


def corner_weights(f):
    """f (m, 3) f32 -> (8, m) f32, ((wx * wy) * wz) with every operation rounded to f32."""
    one = np.float32(1.0)
    out = np.empty((8, f.shape[0]), np.float32)
    for c in range(8):
        wx = f[:, 0] if c & 1 else one - f[:, 0]
        wy = f[:, 1] if (c >> 1) & 1 else one - f[:, 1]
        wz = f[:, 2] if c >> 2 else one - f[:, 2]
        out[c] = (wx * wy) * wz
    return out


def unit_positions(x, xyz_min, xyz_max):
    """x (n, 3) f32 -> x01 (n, 3) f32.  Refuses extents that are not powers of two (see the module docstring)."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 3)
    mn = np.asarray(xyz_min, np.float32).reshape(3)
    ext = np.asarray(xyz_max, np.float32).reshape(3) - mn
    mant, _ = np.frexp(ext)
    if not np.all(mant == 0.5):
        raise ValueError("box extent %r is not a power of two: the kernel's reciprocal is 1 ulp off there, this reference does not cover it" % (ext,))
    inv = np.float32(1.0) / ext
    return (x - mn) * inv                                            # two f32 operations, the second exact


def table_backward_reference(x, xyz_min, xyz_max, dfeats, resolution, offset, scale, active_idx=None, n_active=None, keep_terms=True):
    """x (n_x, 3) f32; dfeats (L, n_samples, 2) f16; resolution / scale (L,), offset (L + 1,).

    n_active (optional int): only the first min(n_active, n_samples) columns of dfeats are live.  active_idx (optional int array,
    needs n_active): live column j belongs to the point x[active_idx[j]]; without it, to x[j].

    Returns Q (total, 2) int64, n_e (total,) contributions per entry, M_e (total, 2) f64 = sum |q| * 2^-24, f16_exact (total, 2) f16,
    hashed (L,) and -- keep_terms -- levels: per level the live columns that contribute (j), their cell, and per corner idx and q."""
    dfeats = np.asarray(dfeats)
    assert dfeats.dtype == np.float16 and dfeats.ndim == 3 and dfeats.shape[2] == 2
    n_levels, n_samples = dfeats.shape[0], dfeats.shape[1]
    assert len(resolution) >= n_levels and len(scale) >= n_levels and len(offset) >= n_levels + 1
    assert active_idx is None or n_active is not None
    live = n_samples if n_active is None else max(0, min(int(n_active), n_samples))
    cols = np.arange(live)
    src = cols if active_idx is None else np.asarray(active_idx)[:live].astype(np.int64)
    x01_all = unit_positions(x, xyz_min, xyz_max)
    assert live == 0 or (src.min() >= 0 and src.max() < x01_all.shape[0])
    x01 = x01_all[src]
    total = int(offset[n_levels])
    Q = np.zeros((total, 2), np.int64)
    mass = np.zeros((total, 2), np.int64)
    n_e = np.zeros(total, np.int64)
    hashed, levels = [], []
    for l in range(n_levels):
        res, off, size = int(resolution[l]), int(offset[l]), int(offset[l + 1]) - int(offset[l])
        hashed.append(is_hashed(res, size))
        g = dfeats[l, :live]
        keep = (g[:, 0] != 0) | (g[:, 1] != 0)                      # -0.0 == 0: such rows contribute nothing
        j = cols[keep]
        pos = fma_f32(x01[keep], np.full((1, 1), scale[l], np.float32), 0.5)
        fl = np.floor(pos)
        f = pos - fl                                                 # exact
        cell = fl.astype(np.int64).astype(np.uint32)                 # (uint32_t)(int)floorf(pos)
        idx = corner_indices(cell, res, size, hashed[l])
        w = corner_weights(f)
        g32 = g[keep].astype(np.float32)
        prod = w[:, :, None] * g32[None, :, :]                       # f32(w * f32(g)), (8, m, 2)
        q = np.rint(prod.astype(np.float64) * FIX_ONE).astype(np.int64)
        for c in range(8):
            np.add.at(n_e, off + idx[c], 1)
            for k in range(2):
                np.add.at(Q[:, k], off + idx[c], q[c, :, k])
                np.add.at(mass[:, k], off + idx[c], np.abs(q[c, :, k]))
        if keep_terms:
            levels.append(SimpleNamespace(j=j, cell=cell, idx=idx, q=q, offset=off, size=size, res=res, hashed=hashed[l]))
    return SimpleNamespace(Q=Q, n_e=n_e, M_e=mass.astype(np.float64) / FIX_ONE, f16_exact=write_out(Q), hashed=hashed, levels=levels)


def write_out(Q):
    """int64 sums -> the f16 the gradient table holds: (float)acc * 2^-24, clamped to +-65504, converted to f16; the int64 -> f32 and
    the f32 -> f16 conversions both round to nearest even."""
    v = Q.astype(np.float32) * np.float32(1.0 / FIX_ONE)
    return np.clip(v, np.float32(-F16_MAX), np.float32(F16_MAX)).astype(np.float16)


def ulp16(v):
    """Spacing of f16 at |v| (2^-24 for zero and the subnormals, 32 in the top binade)."""
    a = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -14)
    _, e = np.frexp(a)                                               # a = m * 2^e, m in [0.5, 1)
    return np.ldexp(1.0, e - 1 - 10)


def ulp32(v):
    """Spacing of f32 at |v| >= 2^-126."""
    _, e = np.frexp(np.abs(np.asarray(v, np.float64)))
    return np.ldexp(1.0, e - 1 - 23)
