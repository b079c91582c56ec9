"""Plain numpy restatement of libngp_meshatlas.so (ngp_pl_amd/csrc/meshatlas/ngp_meshatlas.h, THE RULE), expression for expression: every product
and sum below is one f32 operation in the header's order (no `@`, no fused multiply-add), divisions and square roots are numpy's
correctly rounded ones.  `face_classes`, `sort_faces`, `layout`, `place`, `owners`, `texel_points`, `face_uvs`, `bake`, `sample`,
`render`, and the scene of the acceptance test.  What is identical to the uniform atlas (the key buffer, the quantisation, the
shared scenes) comes from tests/mesh_texture_reference.py.  Test infrastructure only."""
import numpy as np

from tests import mesh_texture_reference as TR
from tests.mesh_visibility_reference import _edge, project

F = np.float32
MAX_WH = 16384
NC = 16
LADDER = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256)
NO_KEY = TR.NO_KEY


def face_classes(vertices, faces, s, cmin=0, cmax=15):
    """(F,) u8: the class of every face from its longest squared edge."""
    if not (np.isfinite(s) and s > 0 and 0 <= cmin <= cmax <= 15):
        raise ValueError("texel_size finite and > 0, 0 <= cmin <= cmax <= 15")
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n_v, s = len(vertices), F(s)
    ok = ((faces >= 0) & (faces < n_v)).all(1)
    cls = np.full(len(faces), cmin, np.uint8)
    k = np.nonzero(ok)[0]
    if not len(k):
        return cls
    A, B, C = [vertices[faces[k, m]] for m in range(3)]

    def e(p, q):
        d = q - p
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]

    with np.errstate(all="ignore"):
        eab, ebc, eca = e(A, B), e(B, C), e(C, A)
        m = eab.copy()
        m = np.where(ebc > m, ebc, m)
        m = np.where(eca > m, eca, m)
        out = np.full(len(k), cmax, np.int64)
        for c in range(cmax, cmin - 1, -1):
            t = F(LADDER[c]) * s
            out = np.where(m <= t * t, c, out)
        out = np.where(np.isfinite(m), out, cmin)
    cls[k] = out
    return cls


def sort_faces(cls):
    """order (F,) i32 by class descending, face index ascending inside a class; counts (16,) i64."""
    cls = np.asarray(cls, np.int64)
    counts = np.bincount(cls, minlength=NC).astype(np.int64)
    order = np.argsort(-cls, kind="stable").astype(np.int32)
    return order, counts


def bases(counts):
    counts = np.asarray(counts, np.int64)
    return np.concatenate([np.cumsum(counts[::-1])[::-1][1:], [0]]).astype(np.int64)


def height_at(counts, W):
    H = 0
    for c in range(NC):
        if counts[c]:
            cpr, cells = W // (LADDER[c] + 5), (int(counts[c]) + 1) // 2
            H += -(-cells // cpr) * (LADDER[c] + 4)
    return H


def layout(counts):
    """(W, H, bands): bands[c] = (y, h, cells_per_row, cells), zeros for an empty class.  ValueError for bad counts, OverflowError
    where the library returns NGP_ERANGE.  A linear search from the smallest width: the definition, not the library's bisection."""
    counts = [int(c) for c in counts]
    if len(counts) != NC or min(counts) < 0 or sum(counts) < 1:
        raise ValueError("16 counts >= 0 with a positive sum")
    if sum(counts) > 2 ** 31 - 1:
        raise OverflowError("more than INT32_MAX faces")
    top = max(c for c in range(NC) if counts[c])
    W = LADDER[top] + 5
    if height_at(counts, MAX_WH) > MAX_WH:
        raise OverflowError("atlas wider than %d texels" % MAX_WH)
    while height_at(counts, W) > W:
        W += 1
    bands, y = [(0, 0, 0, 0)] * NC, 0
    for c in range(NC - 1, -1, -1):
        if counts[c]:
            cpr, cells = W // (LADDER[c] + 5), (counts[c] + 1) // 2
            h = -(-cells // cpr) * (LADDER[c] + 4)
            bands[c] = (y, h, cpr, cells)
            y += h
    return W, y, bands


def place(order, counts):
    """(F, 2) i32: [0] = ox | oy << 16, [1] = c | slot << 8."""
    W, H, bands = layout(counts)
    base = bases(counts)
    order = np.asarray(order, np.int64)
    out = np.zeros((len(order), 2), np.int32)
    for c in range(NC):
        n = int(counts[c])
        if not n:
            continue
        y, h, cpr, cells = bands[c]
        T = LADDER[c]
        q = np.arange(n, dtype=np.int64)
        g, slot = q >> 1, q & 1
        ox, oy = (g % cpr) * (T + 5), y + (g // cpr) * (T + 4)
        f = order[base[c]:base[c] + n]
        out[f, 0] = (ox | (oy << 16)).astype(np.int32)
        out[f, 1] = (c | (slot << 8)).astype(np.int32)
    return out


def decode(face_place):
    """ox, oy, c, slot, T by the header's masks, whatever the record holds."""
    p = np.asarray(face_place, np.int32).reshape(-1, 2).view(np.uint32).astype(np.int64)
    c = p[:, 1] & 15
    return p[:, 0] & 0xFFFF, (p[:, 0] >> 16) & 0xFFFF, c, (p[:, 1] >> 8) & 1, np.asarray(LADDER, np.int64)[c]


def owners(order, counts, begin=0, count=None):
    """Per texel begin .. begin+count-1 of the row-major atlas: face (-1 where there is none), slot coordinates i', j', T."""
    W, H, bands = layout(counts)
    base = bases(counts)
    order = np.asarray(order, np.int64)
    count = W * H - begin if count is None else count
    g = begin + np.arange(count, dtype=np.int64)
    row, col = g // W, g % W
    face = np.full(count, -1, np.int64)
    ip, jp, Tt = np.zeros(count, np.int64), np.zeros(count, np.int64), np.ones(count, np.int64)
    for c in range(NC):
        n = int(counts[c])
        if not n:
            continue
        y, h, cpr, cells = bands[c]
        T = LADDER[c]
        k = np.nonzero((row >= y) & (row < y + h))[0]
        cy, j = (row[k] - y) // (T + 4), (row[k] - y) % (T + 4)
        cx, i = col[k] // (T + 5), col[k] % (T + 5)
        cell = cy * cpr + cx
        slot1 = i + j > T + 3
        q = 2 * cell + slot1
        ok = (cx < cpr) & (cell < cells) & (q < n)
        f = order[np.where(ok, base[c] + q, 0)]
        ok &= (f >= 0) & (f < len(order))
        face[k] = np.where(ok, f, -1)
        ip[k], jp[k], Tt[k] = np.where(slot1, T + 4 - i, i), np.where(slot1, T + 3 - j, j), T
    return face, ip, jp, Tt


def texel_points(vertices, faces, normals, order, counts, box, begin=0, count=None):
    """points (n, 3) f32, dirs (n, 3) f32, valid (n,) u8 of the texels begin .. begin+count-1."""
    vertices, normals = np.asarray(vertices, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    box = np.asarray(box, F).reshape(6)
    n_v = len(vertices)
    face, ip, jp, Tt = owners(order, counts, begin, count)
    n = len(face)
    points = np.tile(box[:3], (n, 1)).astype(F)
    dirs = np.tile(F([0, 0, 1]), (n, 1))
    ok = face >= 0
    fv = faces[np.where(ok, face, 0)]
    ok &= ((fv >= 0) & (fv < n_v)).all(1)
    k = np.nonzero(ok)[0]
    valid = np.zeros(n, np.uint8)
    if not len(k):
        return points, dirs, valid
    a, b, c = [fv[k, m] for m in range(3)]
    u = ((ip[k] - 1).astype(F) / Tt[k].astype(F))[:, None]
    v = ((jp[k] - 1).astype(F) / Tt[k].astype(F))[:, None]
    with np.errstate(all="ignore"):
        A, B, C = vertices[a], vertices[b], vertices[c]
        p = (A + u * (B - A)) + v * (C - A)
        fin = np.isfinite(p).all(1)
        p = np.minimum(np.maximum(p, box[:3]), box[3:])
        NA, NB, NCn = normals[a], normals[b], normals[c]
        nn = (NA + u * (NB - NA)) + v * (NCn - NA)
        L = np.sqrt((nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1]) + nn[:, 2] * nn[:, 2])
        d = -(nn / L[:, None])
        good = (L > 0) & np.isfinite(d).all(1)
    d = np.where(good[:, None], d, F([0, 0, 1])).astype(F)
    k = k[fin]
    points[k], dirs[k] = p[fin], d[fin]
    valid[k] = 1
    return points, dirs, valid


def corner_texels(face_place):
    """(F, 3, 2) int64: the atlas texel (gi, gj) of the corners a, b, c of every face."""
    ox, oy, _, slot, T = decode(face_place)
    out = np.empty((len(ox), 3, 2), np.int64)
    for k, (i, j) in enumerate(((1, 1), (1 + T, 1), (1, 1 + T))):
        out[:, k, 0] = ox + np.where(slot == 1, T + 4 - i, i)
        out[:, k, 1] = oy + np.where(slot == 1, T + 3 - j, j)
    return out


def face_uvs(face_place, W, H):
    """(F, 3, 2) f32."""
    g = corner_texels(face_place).astype(np.float64)
    return np.stack([(g[..., 0] + 0.5) / float(W), 1.0 - (g[..., 1] + 0.5) / float(H)], -1).astype(F)


class Atlas:
    """Everything the restatement derives from a mesh and (s, cmin, cmax), computed once."""

    def __init__(self, vertices, faces, s, cmin=0, cmax=15):
        self.s, self.cmin, self.cmax = s, cmin, cmax
        self.face_class = face_classes(vertices, faces, s, cmin, cmax)
        self.order, self.counts = sort_faces(self.face_class)
        self.W, self.H, self.bands = layout(self.counts)
        self.face_place = place(self.order, self.counts)
        self.uvs = face_uvs(self.face_place, self.W, self.H)
        self.face_texels = np.asarray(LADDER, np.int64)[self.face_class]


def bake(vertices, faces, normals, atlas, box, color_fn):
    """(H, W, 3) u8: color_fn(points, dirs) -> (n, 3) at every texel, quantised."""
    p, d, valid = texel_points(vertices, faces, normals, atlas.order, atlas.counts, box)
    return TR.quantise(color_fn(p, d), valid).reshape(atlas.H, atlas.W, 3)


def sample(texture, face_place, W, H, face, beta, gamma):
    """(n, 3) f32: the bilinear lookup of the rule at (beta, gamma) of each `face`; and the four texels it reads with their weights
    (i0, i1, j0, j1, fx, fy)."""
    face = np.asarray(face, np.int64)
    beta, gamma = np.asarray(beta, F), np.asarray(gamma, F)
    ox, oy, _, slot, T = [a[face] for a in decode(face_place)]
    slot1 = slot == 1
    oxf, oyf = ox.astype(F), oy.astype(F)
    xs, ys = F(1) + beta * T.astype(F), F(1) + gamma * T.astype(F)
    X = np.where(slot1, oxf + ((T + 4).astype(F) - xs), oxf + xs).astype(F)
    Y = np.where(slot1, oyf + ((T + 3).astype(F) - ys), oyf + ys).astype(F)
    flx, fly = np.floor(X), np.floor(Y)
    fx, fy = X - flx, Y - fly
    i0 = np.minimum(np.maximum(flx.astype(np.int64), 0), W - 1)
    j0 = np.minimum(np.maximum(fly.astype(np.int64), 0), H - 1)
    i1, j1 = np.minimum(i0 + 1, W - 1), np.minimum(j0 + 1, H - 1)
    out = None
    if texture is not None:
        t = np.asarray(texture, np.uint8).reshape(H, W, 3).astype(F)
        fxc, fyc = fx[:, None], fy[:, None]
        top = t[j0, i0] * (F(1) - fxc) + t[j0, i1] * fxc
        bot = t[j1, i0] * (F(1) - fxc) + t[j1, i1] * fxc
        out = ((top * (F(1) - fyc) + bot * fyc) / F(255)).astype(F)
    return out, (i0, i1, j0, j1, fx, fy)


def render(vertices, faces, face_place, texture, K, poses, img_wh, near, background=(1, 1, 1), keys=None, return_weights=False):
    """image (C, H, W, 3) f32, face_index (C, H, W) i32, depth (C, H, W) f32 [, beta, gamma (C, H, W) f32, NaN where empty]; the
    texture is (H_atlas, W_atlas, 3) u8."""
    W, H = img_wh
    texture = np.asarray(texture, np.uint8)
    AH, AW = texture.shape[:2]
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    poses = np.asarray(poses, F)
    if keys is None:
        keys = TR.key_buffers(vertices, faces, K, poses, img_wh, near)
    n_c = len(poses)
    image = np.empty((n_c, H, W, 3), F)
    image[:] = np.asarray(background, F)
    face_index = np.full((n_c, H, W), -1, np.int32)
    depth = np.full((n_c, H, W), np.inf, F)
    betas, gammas = np.full((n_c, H, W), np.nan, F), np.full((n_c, H, W), np.nan, F)
    for ci in range(n_c):
        kb = keys[ci].reshape(-1)
        pix = np.nonzero(kb != NO_KEY)[0]
        if not len(pix):
            continue
        f = (kb[pix] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        z = (kb[pix] >> np.uint64(32)).astype(np.uint32).view(F)
        u, v, d = project(vertices, K, poses[ci])
        with np.errstate(all="ignore"):
            q = F(1) / d
            a, b, c = faces[f, 0], faces[f, 1], faces[f, 2]
            px, py = (pix % W).astype(F) + F(0.5), (pix // W).astype(F) + F(0.5)
            wa = _edge(u[b], v[b], u[c], v[c], px, py)
            wb = _edge(u[c], v[c], u[a], v[a], px, py)
            wc = _edge(u[a], v[a], u[b], v[b], px, py)
            la, lb, lc = wa * q[a], wb * q[b], wc * q[c]
            s = (la + lb) + lc
            beta = np.minimum(np.maximum(lb / s, F(0)), F(1))
            gamma = np.minimum(np.maximum(lc / s, F(0)), F(1))
        colour, _ = sample(texture, face_place, AW, AH, f, beta, gamma)
        image[ci].reshape(-1, 3)[pix] = colour
        face_index[ci].reshape(-1)[pix] = f
        depth[ci].reshape(-1)[pix] = z
        betas[ci].reshape(-1)[pix], gammas[ci].reshape(-1)[pix] = beta, gamma
    return (image, face_index, depth, betas, gammas) if return_weights else (image, face_index, depth)


def fit_texel_size(vertices, faces, max_side, cmin=0, cmax=15, probes=24):
    """ngp_pl_amd.mesh.fit_texel_size, step for step: the bisection on log2(texel_size), every probe rounded to f32."""
    import math
    vertices = np.asarray(vertices, F).reshape(-1, 3)

    def fits(s):
        try:
            W, H, _ = layout(sort_faces(face_classes(vertices, faces, s, cmin, cmax))[1])
        except OverflowError:
            return False
        return max(W, H) <= max_side

    longest = 4.0 * float(np.abs(np.nan_to_num(vertices, nan=0.0, posinf=0.0, neginf=0.0)).max()) if len(vertices) else 1.0
    longest = longest if math.isfinite(longest) and longest > 0 else 1.0
    hi = math.log2(longest) + 1.0
    lo = hi - 40.0
    best = float(F(2.0 ** hi))
    if not fits(best):
        raise ValueError("does not fit")
    for _ in range(probes):
        mid = 0.5 * (lo + hi)
        s = float(F(2.0 ** mid))
        if fits(s):
            best, hi = s, mid
        else:
            lo = mid
    return best


# ---- measures and scenes ----------------------------------------------------------------------------------------------------

def longest_edges(vertices, faces):
    """(F,) f64: the longest edge of every face."""
    p = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return np.sqrt(((p - p[:, [1, 2, 0]]) ** 2).sum(2)).max(1)


def face_spacing(vertices, faces, face_texels):
    """(F,) f64: world units per texel interval along the longest edge of every face."""
    return longest_edges(vertices, faces) / np.asarray(face_texels, np.float64)


def box_and_ball(n=7, half=0.42, radius=0.14, centre=(0.0, 0.0, 0.62)):
    """One mesh of two parts inside [-1, 1]^3 that the cameras of TR.sphere_cameras both see: a box of 12 faces with half-side
    `half` round the origin, outward normals per corner, and the marching-cubes sphere of TR.sphere_mesh(n) shrunk to `radius` beside
    it at `centre`: a few faces carry most of the area.  vertices, faces, normals."""
    corners = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]        # outward
    bf = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    bv = (corners * half).astype(F)
    bn = (corners / np.sqrt(3.0)).astype(F)
    sv, sf, sn = TR.sphere_mesh(n, radius=0.7, jitter=0.1, seed=3)
    sv = (sv.astype(np.float64) * (radius / 0.7) + np.asarray(centre)).astype(F)
    v = np.concatenate([bv, sv])
    f = np.concatenate([bf, sf.astype(np.int32) + len(bv)]).astype(np.int32)
    return v, f, np.concatenate([bn, sn]).astype(F)


def wave_colour(period):
    """color_fn(points, dirs): 0.5 + 0.4 sin(2 pi x_k / period) per channel k, in f64 rounded to f32: smooth in space."""
    def fn(points, dirs=None):
        p = np.asarray(points, np.float64)
        return (0.5 + 0.4 * np.sin(2.0 * np.pi * p / period)).astype(F)
    return fn
