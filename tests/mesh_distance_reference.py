"""Test infrastructure, no GPU: the rule of include/ngp_meshdist.h restated in numpy.

  sample_f32      rule 1, the surface samples, operation by operation in float32.
  closest_f32     rule 2, the region test vectorised over point x face pairs, in float32.
  query_f32       rule 3, the brute-force minimum of the key  bits(d2) << 32 | face  over every face.
  distance_f64    the definition by an independent route in float64: project onto the plane, test inside, else the minimum of the
                  three clamped segment distances.
  stats_fsum      rule 4 with math.fsum.
  slack, cell_of  the grid's slack and cell index, for tests that place queries on purpose.
"""
import math

import numpy as np

F = np.float32
K_MAX = 64
SLACK_ULPS = 64
U = 2.0 ** -24


def slack(m):
    return F(F(SLACK_ULPS * 2.0 ** -23) * F(m))


def cell_of(t, o, cell, n):
    with np.errstate(all="ignore"):
        g = np.floor((F(t) - F(o)) / F(cell))
    if not g >= 0:
        return 0
    return n - 1 if g >= n else int(g)


def usable(v, f):
    """Bool (F,): the indices are in range and the nine coordinates are finite."""
    v, f = np.asarray(v, F).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    if len(v):
        ok &= np.isfinite(v[np.clip(f, 0, len(v) - 1)]).all((1, 2))
    return ok


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def subdivision(a, b, c, spacing):
    """k of rule 1 for triangles (n, 3) f32."""
    with np.errstate(all="ignore"):
        ab, ac, bc = b - a, c - a, c - b
        longest = np.maximum(np.maximum(np.sqrt(_dot(ab, ab)), np.sqrt(_dot(ac, ac))), np.sqrt(_dot(bc, bc)))
        q = np.ceil(longest / F(spacing))
    k = np.where(q >= K_MAX, K_MAX, np.where(q >= 1, q, 1))
    return np.where(np.isnan(q), 1, k).astype(np.int64)


def barycentric_integers(k, s):
    r = math.isqrt(s)
    col = s - r * r
    t = col // 2
    if col % 2 == 0:
        return 3 * (k - r) - 2, 3 * (r - t) + 1, 3 * t + 1
    return 3 * (k - r) - 1, 3 * (r - t) - 1, 3 * t + 2


def sample_f32(v, f, spacing):
    """points (S, 3) f32, weights (S,) f32, face ids (S,) i32 and the per-face counts (F,) i64."""
    v, f = np.asarray(v, F).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    ok = usable(v, f)
    counts = np.zeros(len(f), np.int64)
    pts, wts, ids = [], [], []
    for face in np.nonzero(ok)[0]:
        a, b, c = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
        k = int(subdivision(a[None], b[None], c[None], spacing)[0])
        counts[face] = k * k
        ijl = np.array([barycentric_integers(k, s) for s in range(k * k)], np.int64)
        i, j, l = (ijl[:, n].astype(F)[:, None] for n in range(3))
        with np.errstate(all="ignore"):
            pts.append(((i * a[None] + j * b[None]) + l * c[None]) / F(3 * k))
            ab, ac = b - a, c - a
            n = np.array([ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]], F)
            w = (F(0.5) * np.sqrt(_dot(n, n))) / F(k * k)
        wts.append(np.full(k * k, w, F))
        ids.append(np.full(k * k, face, np.int32))
    if not pts:
        return np.zeros((0, 3), F), np.zeros(0, F), np.zeros(0, np.int32), counts
    return np.concatenate(pts).astype(F), np.concatenate(wts), np.concatenate(ids), counts


def closest_f32(p, a, b, c):
    """Rule 2 for every pair: p (n, 3), a, b, c (m, 3) f32 -> q (n, m, 3) f32, d2 (n, m) f32 and the case (n, m) i8
    (0 a, 1 b, 2 ab, 3 c, 4 ac, 5 bc, 6 interior)."""
    p = np.asarray(p, F).reshape(-1, 1, 3)
    a, b, c = (np.asarray(x, F).reshape(1, -1, 3) for x in (a, b, c))
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        s43, s56 = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (s43 >= 0) & (s56 >= 0)]
        shape = np.broadcast(p, a).shape
        full = lambda x: np.broadcast_to(x, shape)
        v_ab = (d1 / (d1 - d3))[..., None]
        w_ac = (d2 / (d2 - d6))[..., None]
        w_bc = (s43 / (s43 + s56))[..., None]
        denom = F(1) / ((va + vb) + vc)
        v, w = vb * denom, vc * denom
        v = np.where(v >= 0, v, F(0))
        v = np.where(v > 1, F(1), v)
        w = np.where(w >= 0, w, F(0))
        rest = F(1) - v
        w = np.where(w > rest, rest, w)
        qs = [full(a), full(b), a + v_ab * ab, full(c), a + w_ac * ac, b + w_bc * (c - b), (a + v[..., None] * ab) + w[..., None] * ac]
        case = np.full(shape[:2], 6, np.int8)
        q = qs[6].astype(F)
        for k in range(5, -1, -1):
            case = np.where(conds[k], np.int8(k), case)
            q = np.where(conds[k][..., None], qs[k], q)
        e = p - q
        dd = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    return q.astype(F), dd.astype(F), case


def query_f32(points, v, f, max_dist=np.inf, chunk=256):
    """Rule 3 by brute force: d2 (n,) f32, face (n,) i32, q (n, 3) f32."""
    points, v, f = np.asarray(points, F).reshape(-1, 3), np.asarray(v, F).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    n = len(points)
    out_d2, out_face, out_q = np.full(n, np.inf, F), np.full(n, -1, np.int32), np.full((n, 3), np.nan, F)
    faces = np.nonzero(usable(v, f))[0]
    if len(faces) == 0 or n == 0:
        return out_d2, out_face, out_q
    a, b, c = (v[f[faces, k]] for k in range(3))
    with np.errstate(all="ignore"):
        md2 = F(max_dist) * F(max_dist)
    for begin in range(0, n, chunk):
        q, dd, _ = closest_f32(points[begin:begin + chunk], a, b, c)
        key = (dd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | faces.astype(np.uint64)[None]
        key = np.where(np.isfinite(dd), key, np.uint64(0xFFFFFFFFFFFFFFFF))
        at = key.argmin(1)
        rows = np.arange(len(at))
        best = key[rows, at]
        hit = (best != np.uint64(0xFFFFFFFFFFFFFFFF)) & ~(dd[rows, at] > md2)
        sl = slice(begin, begin + len(at))
        out_d2[sl] = np.where(hit, dd[rows, at], F(np.inf))
        out_face[sl] = np.where(hit, faces[at], -1)
        out_q[sl] = np.where(hit[:, None], q[rows, at], F(np.nan))
    return out_d2, out_face, out_q


def _segment_f64(p, a, b):
    ab = b - a
    den = float(ab @ ab)
    t = 0.0 if den == 0.0 else min(1.0, max(0.0, float((p - a) @ ab) / den))
    return float(np.linalg.norm(p - (a + t * ab)))


def distance_f64(p, a, b, c):
    """The distance from p to the triangle (a, b, c), all (3,), in float64: the foot of the perpendicular if it lies inside,
    else the nearest of the three edges."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    n = np.cross(b - a, c - a)
    nn = float(n @ n)
    if nn > 0.0:
        foot = p - n * (float((p - a) @ n) / nn)
        inside = all(float(np.cross(y - x, foot - x) @ n) >= 0.0 for x, y in ((a, b), (b, c), (c, a)))
        if inside:
            return abs(float((p - a) @ n)) / math.sqrt(nn)
    return min(_segment_f64(p, a, b), _segment_f64(p, b, c), _segment_f64(p, c, a))


def lower_error(m):
    """E of the header: sqrt(computed d2) >= distance - E, for coordinates of magnitude <= m."""
    return 33.0 * U * m


def upper_error(p, a, b, c):
    """The header's other side: sqrt(computed d2) <= distance + 2E + min(L, 32 u L^3 D^2 / area^2)."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    m = max(np.abs(x).max() for x in (p, a, b, c))
    L = max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b))
    D = max(np.linalg.norm(p - a), np.linalg.norm(p - b), np.linalg.norm(p - c))
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a))
    shape = 32.0 * U * L ** 3 * D ** 2 / area ** 2 if area > 0 else np.inf
    return 2.0 * lower_error(m) + min(L, shape)


def stats_fsum(d2, face, weights, thresholds=()):
    """Rule 4's 14 numbers with exactly rounded sums, and the sum of |term| behind each of them (for the f64 bound)."""
    d2, face, weights = np.asarray(d2, F), np.asarray(face, np.int64), np.asarray(weights, F)
    hit = face >= 0
    w = weights.astype(np.float64)
    with np.errstate(all="ignore"):
        d = np.sqrt(d2).astype(np.float64)
    terms = [w[hit], w[hit] * d[hit], w[hit] * d2[hit].astype(np.float64), None, w[~hit], np.ones(int((~hit).sum()))]
    for t in range(8):
        if t < len(thresholds):
            tt = F(thresholds[t]) * F(thresholds[t])
            terms.append(w[hit & (d2 <= tt)])
        else:
            terms.append(np.zeros(0))
    out = [math.fsum(x) if x is not None else (float(d[hit].max()) if hit.any() else 0.0) for x in terms]
    mag = [math.fsum(np.abs(x)) if x is not None else 0.0 for x in terms]
    return out, mag
