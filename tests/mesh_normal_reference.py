"""Test infrastructure, no GPU: the rule of ngp_pl_amd/csrc/meshnormal/ngp_meshnormal.h restated in numpy.

  eligible_f32    rule 1, usable faces and the orientation test dot(g, m) > 0, for every query x face pair, in float32.
  pair_f32        rule 2 for one face per query: q, d2, the deciding case and its barycentric pair (v, w), in float32.
  transfer_f32    rules 3 and 4 by brute force over every face: normals, d2, face, bary.
  transfer_f64    the definition by an independent route in float64: the foot of the perpendicular if it lies inside, else the
                  nearest of the three clamped segments; barycentrics from the closest point; the orientation test; the normal.
  shade_f32       rule 5.
  bake_image, decode, angles   the normal-map image and what a viewer reads back from it.
  the scenes      the thin wall, a lattice of squares in two sheets, the rippled sheet, icospheres.
"""
import numpy as np

from tests import mesh_distance_reference as DR
from tests import mesh_texture_reference as TR

F = np.float32
MAX_SHELLS = 8
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
FMAX = F(3.402823466e38)


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def eligible_f32(v, f, m, oriented):
    """Bool (n, F): face j is eligible for query i (rule 1)."""
    v, f, m = np.asarray(v, F).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3), np.asarray(m, F).reshape(-1, 3)
    ok = DR.usable(v, f)
    out = np.broadcast_to(ok[None], (len(m), len(f))).copy()
    if oriented and len(f) and len(v):
        fc = np.clip(f, 0, len(v) - 1)
        a, b, c = v[fc[:, 0]], v[fc[:, 1]], v[fc[:, 2]]
        with np.errstate(all="ignore"):
            ab, ac = b - a, c - a
            g = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2],
                          ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], 1).astype(F)
            dots = (g[None, :, 0] * m[:, None, 0] + g[None, :, 1] * m[:, None, 1]) + g[None, :, 2] * m[:, None, 2]
            out &= dots > 0
    return out


def pair_f32(p, a, b, c):
    """Rule 2 for query i against triangle i: p, a, b, c (n, 3) f32 -> q (n, 3), d2 (n,), case (n,) i8 (0 a, 1 b, 2 ab, 3 c, 4 ac,
    5 bc, 6 interior), v (n,), w (n,), all f32."""
    p, a, b, c = (np.asarray(x, F).reshape(-1, 3) for x in (p, a, b, c))
    one, zero = F(1), F(0)
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
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = s43 / (s43 + s56)
        denom = one / ((va + vb) + vc)
        v, w = vb * denom, vc * denom
        v = np.where(v >= 0, v, zero)
        v = np.where(v > 1, one, v)
        w = np.where(w >= 0, w, zero)
        rest = one - v
        w = np.where(w > rest, rest, w)
        z, o = np.zeros_like(d1), np.ones_like(d1)
        qs = [a, b, a + v_ab[:, None] * ab, c, a + w_ac[:, None] * ac, b + w_bc[:, None] * (c - b), (a + v[:, None] * ab) + w[:, None] * ac]
        vs = [z, o, v_ab, z, z, one - w_bc, v]
        ws = [z, z, z, o, w_ac, w_bc, w]
        case = np.full(len(p), 6, np.int8)
        q, bv, bw = qs[6].astype(F), vs[6], ws[6]
        for k in range(5, -1, -1):
            case = np.where(conds[k], np.int8(k), case)
            q = np.where(conds[k][:, None], qs[k], q)
            bv, bw = np.where(conds[k], vs[k], bv), np.where(conds[k], ws[k], bw)
        e = p - q
        dd = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    return q.astype(F), dd.astype(F), case, bv.astype(F), bw.astype(F)


def fallback_f32(m):
    """Rule 4's fallback: m / |m|, or (0, 0, 1)."""
    m = np.asarray(m, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        L = np.sqrt(_dot(m, m))
        good = (L > 0) & (L <= FMAX)
        out = m / L[:, None]
    return np.where(good[:, None], out, F([0, 0, 1])).astype(F)


def transfer_f32(points, qnormals, valid, v, f, vn, max_dist, oriented=True, chunk=256):
    """Rules 1 to 4 by brute force over every face: normals (n, 3) f32, d2 (n,) f32, face (n,) i32, bary (n, 2) f32."""
    points, qnormals = np.asarray(points, F).reshape(-1, 3), np.asarray(qnormals, F).reshape(-1, 3)
    v, vn, f = np.asarray(v, F).reshape(-1, 3), np.asarray(vn, F).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    n = len(points)
    valid = np.ones(n, np.uint8) if valid is None else np.asarray(valid, np.uint8)
    live = (valid != 0) & np.isfinite(points).all(1)
    out_n, out_d2 = np.zeros((n, 3), F), np.full(n, np.inf, F)
    out_face, out_bary = np.full(n, -1, np.int32), np.zeros((n, 2), F)
    out_n[live] = fallback_f32(qnormals[live])
    faces = np.nonzero(DR.usable(v, f))[0]
    idx = np.nonzero(live)[0]
    if len(faces) == 0 or len(idx) == 0:
        return out_n, out_d2, out_face, out_bary
    a, b, c = (v[f[faces, k]] for k in range(3))
    with np.errstate(all="ignore"):
        md2 = F(max_dist) * F(max_dist)
    for begin in range(0, len(idx), chunk):
        rows = idx[begin:begin + chunk]
        _, dd, _ = DR.closest_f32(points[rows], a, b, c)
        key = (dd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | faces.astype(np.uint64)[None]
        ok = np.isfinite(dd) & eligible_f32(v, f, qnormals[rows], oriented)[:, faces]
        key = np.where(ok, key, NO_KEY)
        at = key.argmin(1)
        r = np.arange(len(rows))
        hit = (key[r, at] != NO_KEY) & ~(dd[r, at] > md2)
        win = faces[at[hit]]
        hr = rows[hit]
        _, d2w, _, bv, bw = pair_f32(points[hr], v[f[win, 0]], v[f[win, 1]], v[f[win, 2]])
        assert np.array_equal(d2w.view(np.int32), dd[r, at][hit].view(np.int32))            # the two restatements of rule 2 agree
        na, nb, nc = vn[f[win, 0]], vn[f[win, 1]], vn[f[win, 2]]
        with np.errstate(all="ignore"):
            bu = (F(1) - bv) - bw
            N = (bu[:, None] * na + bv[:, None] * nb) + bw[:, None] * nc
            L = np.sqrt(_dot(N, N))
            good = (L > 0) & (L <= FMAX)
            unit = N / L[:, None]
        out_n[hr] = np.where(good[:, None], unit, out_n[hr]).astype(F)
        out_d2[hr], out_face[hr] = d2w, win
        out_bary[hr] = np.stack([bv, bw], 1)
    return out_n, out_d2, out_face, out_bary


# ---- the float64 definition, by another route


def closest_f64(p, a, b, c):
    """For every pair: p (n, 3), a, b, c (m, 3) -> distance (n, m) and the barycentric pair (v, w) (n, m) of the closest point, in
    float64: the foot of the perpendicular where it lies inside the triangle, else the nearest point of the three edges."""
    p = np.asarray(p, np.float64).reshape(-1, 1, 3)
    a, b, c = (np.asarray(x, np.float64).reshape(1, -1, 3) for x in (a, b, c))
    ab, ac = b - a, c - a
    nrm = np.cross(ab, ac)
    nn = (nrm * nrm).sum(-1)
    with np.errstate(all="ignore"):
        foot = p - nrm * (((p - a) * nrm).sum(-1) / nn)[..., None]
        inside = np.ones(foot.shape[:2], bool)
        for x, y in ((a, b), (b, c), (c, a)):
            inside &= (np.cross(np.broadcast_to(y - x, foot.shape), foot - x) * nrm).sum(-1) >= 0
        inside &= nn > 0
    best = np.where(inside[..., None], foot, np.nan)
    dist = np.where(inside, np.linalg.norm(p - foot, axis=-1), np.inf)
    for x, y in ((a, b), (b, c), (c, a)):
        e = y - x
        den = (e * e).sum(-1)
        with np.errstate(all="ignore"):
            t = np.clip(((p - x) * e).sum(-1) / den, 0.0, 1.0)
        t = np.where(den > 0, t, 0.0)
        q = x + t[..., None] * e
        d = np.linalg.norm(p - q, axis=-1)
        closer = d < dist
        best, dist = np.where(closer[..., None], q, best), np.where(closer, d, dist)
    r = best - a                                                    # q = a + v ab + w ac: the 2 x 2 normal equations
    g11, g12, g22 = (ab * ab).sum(-1), (ab * ac).sum(-1), (ac * ac).sum(-1)
    r1, r2 = (r * ab).sum(-1), (r * ac).sum(-1)
    with np.errstate(all="ignore"):
        det = g11 * g22 - g12 * g12
        bv, bw = (r1 * g22 - r2 * g12) / det, (r2 * g11 - r1 * g12) / det
    return dist, bv, bw


def transfer_f64(points, qnormals, v, f, vn, max_dist, oriented=True):
    """The definition in float64: normals (n, 3), distance (n,), face (n,) i64 (-1: a miss), and the distance to every face (n, F),
    +inf where the face is not eligible."""
    points, qnormals = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(qnormals, np.float64).reshape(-1, 3)
    v64, vn64, f = np.asarray(v, np.float64).reshape(-1, 3), np.asarray(vn, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    a, b, c = v64[f[:, 0]], v64[f[:, 1]], v64[f[:, 2]]
    dist, bv, bw = closest_f64(points, a, b, c)
    if oriented:
        g = np.cross(b - a, c - a)
        dist = np.where(qnormals @ g.T > 0, dist, np.inf)
    face = dist.argmin(1)
    r = np.arange(len(points))
    d = dist[r, face]
    hit = d <= max_dist
    bv, bw = bv[r, face], bw[r, face]
    N = (1 - bv - bw)[:, None] * vn64[f[face, 0]] + bv[:, None] * vn64[f[face, 1]] + bw[:, None] * vn64[f[face, 2]]
    with np.errstate(all="ignore"):
        N = N / np.linalg.norm(N, axis=1, keepdims=True)
        own = qnormals / np.linalg.norm(qnormals, axis=1, keepdims=True)
    N = np.where(hit[:, None] & np.isfinite(N).all(1)[:, None], N, own)
    return N, np.where(hit, d, np.inf), np.where(hit, face, -1), dist


# ---- shading, the image


def shade_f32(albedo, samples, ids, lights, ambient):
    """Rule 5: (C, H, W, 3) f32."""
    albedo, samples, lights = np.asarray(albedo, F), np.asarray(samples, F), np.asarray(lights, F)
    amb = F(ambient)
    with np.errstate(all="ignore"):
        t = F(2) * samples - F(1)
        L = np.sqrt(_dot(t, t))
        u = t / L[..., None]
        l = lights[:, None, None, :]
        d = (u[..., 0] * l[..., 0] + u[..., 1] * l[..., 1]) + u[..., 2] * l[..., 2]
        k = amb + (F(1) - amb) * np.where(d > 0, d, F(0))
    k = np.where((L > 0) & (L <= FMAX), k, F(1)).astype(F)
    k = np.where(np.asarray(ids) >= 0, k, F(1))
    out = albedo * k[..., None]
    return np.where((np.asarray(ids) >= 0)[..., None], out, albedo).astype(F)


def light_f32(light):
    l = np.asarray(light, F)
    return l / np.sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2])


def bake_image(points, dirs, valid, v, f, vn, max_dist, oriented=True):
    """The bytes of bake_normal_map for texels (points, dirs, valid): (n, 3) u8, and transfer_f32's outputs."""
    out = transfer_f32(points, -np.asarray(dirs, F), valid, v, f, vn, max_dist, oriented)
    return TR.quantise(out[0] * F(0.5) + F(0.5), valid), out


def decode(image):
    """What a viewer reads: 2 * byte / 255 - 1, normalised, float64."""
    t = 2.0 * np.asarray(image, np.float64) / 255.0 - 1.0
    return t / np.linalg.norm(t, axis=-1, keepdims=True)


def angles(a, b):
    """Degrees between the rows of a and b (unit or not), float64."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a / np.linalg.norm(a, axis=-1, keepdims=True), b / np.linalg.norm(b, axis=-1, keepdims=True)
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), (a * b).sum(-1)))


# ---- the scenes

WALL_GAP = 0.01


def _sheet(nx, ny, step, z, up, origin=(0.0, 0.0)):
    """An nx x ny lattice of squares of edge `step` in the plane z, two triangles each, wound to face +z (up) or -z."""
    xs, ys = origin[0] + np.arange(nx + 1) * step, origin[1] + np.arange(ny + 1) * step
    v = np.array([[x, y, z] for y in ys for x in xs], np.float64)
    f = []
    for j in range(ny):
        for i in range(nx):
            a = j * (nx + 1) + i
            b, c, d = a + 1, a + nx + 1, a + nx + 2
            f += [[a, b, d], [a, d, c]] if (i + j) % 2 == 0 else [[a, b, c], [b, d, c]]
    f = np.array(f, np.int32)
    return v.astype(F), f if up else f[:, ::-1].copy()


def thin_wall():
    """Two unit squares: one at z = 0 wound to face -z, one at z = 0.01 facing +z.  vertices, faces, vertex normals."""
    v0, f0 = _sheet(1, 1, 1.0, 0.0, up=False)
    v1, f1 = _sheet(1, 1, 1.0, WALL_GAP, up=True)
    vn = np.concatenate([np.tile(F([0, 0, -1]), (4, 1)), np.tile(F([0, 0, 1]), (4, 1))])
    return np.concatenate([v0, v1]), np.concatenate([f0, f1 + 4]), vn


def lattice(step=0.25, gap=0.3, origin=(-0.75, -0.75)):
    """6 x 6 x 2 squares: a sheet at z = 0 that faces -z and one at z = gap that faces +z, 144 faces, with unit vertex normals that
    vary over the sheets (so that the interpolation shows)."""
    v0, f0 = _sheet(6, 6, step, 0.0, up=False, origin=origin)
    v1, f1 = _sheet(6, 6, step, gap, up=True, origin=origin)
    v = np.concatenate([v0, v1])
    f = np.concatenate([f0, f1 + len(v0)])
    s = np.where(v[:, 2] > 0.5 * gap, 1.0, -1.0)
    n = np.stack([0.3 * np.sin(3.0 * v[:, 0]), 0.3 * np.cos(2.0 * v[:, 1]), s], 1)
    return v, f, (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)


RIPPLE_A, RIPPLE_PERIOD = 0.01, 0.25


def ripple_sheet():
    """z = 0.01 sin(2 pi x / 0.25) over the unit square on a 65 x 9 grid (1 024 faces, facing +z) with the analytic vertex normals."""
    v, f = _sheet(64, 8, 1.0, 0.0, up=True)
    v = v.astype(np.float64)
    v[:, 0], v[:, 1] = v[:, 0] / 64.0, v[:, 1] / 8.0
    k = 2.0 * np.pi / RIPPLE_PERIOD
    v[:, 2] = RIPPLE_A * np.sin(k * v[:, 0])
    return v.astype(F), f, ripple_normal(v[:, 0]).astype(F)


def ripple_normal(x):
    k = 2.0 * np.pi / RIPPLE_PERIOD
    n = np.stack([-RIPPLE_A * k * np.cos(k * x), np.zeros_like(x), np.ones_like(x)], 1)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def ripple_foot(x0):
    """The x of the point of the curve z = A sin(k x) nearest to (x0, 0), float64, by Newton's method from x0 (A k = 0.25: the
    function (x - x0) + A^2 k sin(k x) cos(k x) is increasing)."""
    k = 2.0 * np.pi / RIPPLE_PERIOD
    x = np.asarray(x0, np.float64).copy()
    for _ in range(20):
        g = (x - x0) + RIPPLE_A ** 2 * k * np.sin(k * x) * np.cos(k * x)
        x = x - g / (1.0 + RIPPLE_A ** 2 * k * k * np.cos(2.0 * k * x))
    return x


def icosphere(subdivisions):
    """The unit icosphere: vertices (V, 3) f32 on the sphere, faces (F, 3) i32 counter-clockwise from outside (20 * 4^s faces), and
    the radial normals."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def middle(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    v = np.asarray(v, np.float64)
    v32 = v.astype(F)
    nrm = (v32.astype(np.float64) / np.linalg.norm(v32.astype(np.float64), axis=1, keepdims=True)).astype(F)
    return v32, np.asarray(f, np.int32), nrm


def barycentric_texels(v, f, vn, T):
    """The (T + 1)(T + 2) / 2 lattice points of every face with their interpolated, normalised vertex normals: points (n, 3) f32,
    normals (n, 3) f32 and the face of each."""
    v, vn, f = np.asarray(v, np.float64), np.asarray(vn, np.float64), np.asarray(f, np.int64)
    ij = [(i, j) for i in range(T + 1) for j in range(T + 1 - i)]
    bv, bw = np.array([x[0] for x in ij]) / T, np.array([x[1] for x in ij]) / T
    bu = 1.0 - bv - bw
    mix = lambda x: (bu[None, :, None] * x[f[:, 0]][:, None] + bv[None, :, None] * x[f[:, 1]][:, None] + bw[None, :, None] * x[f[:, 2]][:, None]).reshape(-1, 3)
    p, n = mix(v), mix(vn)
    return p.astype(F), (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F), np.repeat(np.arange(len(f)), len(ij))


def face_normals(v, f):
    v, f = np.asarray(v, np.float64), np.asarray(f, np.int64)
    g = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return g / np.linalg.norm(g, axis=1, keepdims=True)
