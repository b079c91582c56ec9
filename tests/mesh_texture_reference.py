"""Plain numpy restatement of libngp_meshtex.so (include/ngp_meshtex.h, THE RULE), expression for expression: every product and
sum below is one f32 operation in the header's order (no `@`, no fused multiply-add), divisions and square roots are numpy's
correctly rounded ones.  `atlas_size`, `owners`, `texel_points`, `face_uvs`, `bake`, `key_buffers`, `render`; and the small scenes
the CPU and GPU tests share.  The projection is the one of tests/mesh_visibility_reference.py (the cull's rule), used as it is.
Test infrastructure only."""
import numpy as np

from tests.mesh_visibility_reference import _edge, project

F = np.float32
MAX_WH = 16384
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def atlas_size(n_faces, T):
    """(cells_per_row, W, H); ValueError for bad arguments, OverflowError where the library returns NGP_ERANGE."""
    if n_faces < 1 or not 1 <= T <= 256:
        raise ValueError("n_faces >= 1 and 1 <= T <= 256")
    cw, ch = T + 5, T + 4
    n_cells = (n_faces + 1) // 2
    c = 1
    while c * cw <= MAX_WH:
        rows = -(-n_cells // c)
        if c * cw >= rows * ch:
            return c, c * cw, rows * ch
        c += 1
    raise OverflowError("atlas wider or higher than %d texels" % MAX_WH)


def owners(n_faces, T, begin=0, count=None):
    """Per texel begin .. begin+count-1 of the row-major atlas: face (-1 where the slot has no face), slot coordinates i', j'."""
    c, W, H = atlas_size(n_faces, T)
    cw, ch = T + 5, T + 4
    count = W * H - begin if count is None else count
    g = begin + np.arange(count, dtype=np.int64)
    row, col = g // W, g % W
    cell = (row // ch) * c + col // cw
    i, j = col % cw, row % ch
    slot1 = i + j > T + 3
    ip = np.where(slot1, T + 4 - i, i)
    jp = np.where(slot1, T + 3 - j, j)
    face = 2 * cell + slot1
    face = np.where((cell < (n_faces + 1) // 2) & (face < n_faces), face, -1)
    return face, ip, jp


def texel_points(vertices, faces, normals, T, box, begin=0, count=None):
    """points (n, 3) f32, dirs (n, 3) f32, valid (n,) u8 of the texels begin .. begin+count-1."""
    vertices, normals = np.asarray(vertices, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    box = np.asarray(box, F).reshape(6)
    n_v = len(vertices)
    face, ip, jp = owners(len(faces), T, begin, count)
    n = len(face)
    points = np.tile(box[:3], (n, 1)).astype(F)
    dirs = np.tile(F([0, 0, 1]), (n, 1))
    ok = face >= 0
    fv = faces[np.where(ok, face, 0)]
    ok &= ((fv >= 0) & (fv < n_v)).all(1)
    k = np.nonzero(ok)[0]
    a, b, c = [fv[k, m] for m in range(3)]
    u = ((ip[k] - 1).astype(F) / F(T))[:, None]
    v = ((jp[k] - 1).astype(F) / F(T))[:, None]
    with np.errstate(all="ignore"):
        A, B, C = vertices[a], vertices[b], vertices[c]
        p = (A + u * (B - A)) + v * (C - A)
        fin = np.isfinite(p).all(1)
        p = np.minimum(np.maximum(p, box[:3]), box[3:])
        NA, NB, NC = normals[a], normals[b], normals[c]
        nn = (NA + u * (NB - NA)) + v * (NC - NA)
        L = np.sqrt((nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1]) + nn[:, 2] * nn[:, 2])
        d = -(nn / L[:, None])
        good = (L > 0) & np.isfinite(d).all(1)
    d = np.where(good[:, None], d, F([0, 0, 1])).astype(F)
    k = k[fin]
    points[k], dirs[k] = p[fin], d[fin]
    valid = np.zeros(n, np.uint8)
    valid[k] = 1
    return points, dirs, valid


def corner_texels(n_faces, T):
    """(F, 3, 2) int64: the atlas texel (gi, gj) of the corners a, b, c of every face."""
    c, W, H = atlas_size(n_faces, T)
    f = np.arange(n_faces, dtype=np.int64)
    cell, slot1 = f >> 1, (f & 1) == 1
    ox, oy = (cell % c) * (T + 5), (cell // c) * (T + 4)
    out = np.empty((n_faces, 3, 2), np.int64)
    for k, (i, j) in enumerate(((1, 1), (1 + T, 1), (1, 1 + T))):
        out[:, k, 0] = ox + np.where(slot1, T + 4 - i, i)
        out[:, k, 1] = oy + np.where(slot1, T + 3 - j, j)
    return out


def face_uvs(n_faces, T):
    """(F, 3, 2) f32."""
    _, W, H = atlas_size(n_faces, T)
    g = corner_texels(n_faces, T).astype(np.float64)
    return np.stack([(g[..., 0] + 0.5) / float(W), 1.0 - (g[..., 1] + 0.5) / float(H)], -1).astype(F)


def quantise(colours, valid):
    """(n, 3) f32 colours -> u8: round(clamp(c, 0, 1) * 255), halves to even, 0 for invalid texels."""
    q = np.rint(np.clip(np.asarray(colours, F), F(0), F(1)) * F(255)).astype(np.uint8)
    q[np.asarray(valid) == 0] = 0
    return q


def bake(vertices, faces, normals, T, box, color_fn):
    """(H, W, 3) u8: color_fn(points, dirs) -> (n, 3) at every texel, quantised."""
    _, W, H = atlas_size(len(faces), T)
    p, d, valid = texel_points(vertices, faces, normals, T, box)
    return quantise(color_fn(p, d), valid).reshape(H, W, 3)


def key_buffer(vertices, faces, K, pose, img_wh, near):
    """(H, W) u64: per pixel the minimum of (bits(z) << 32) | face over the faces that cover it, all ones where none does."""
    W, H = img_wh
    n_v = len(vertices)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    kb = np.full(H * W, NO_KEY, np.uint64)
    index = np.nonzero(((faces >= 0) & (faces < n_v)).all(1))[0]
    faces = faces[index]
    if not len(faces):
        return kb.reshape(H, W)
    u, v, d = project(vertices, K, pose)
    near = F(near)
    with np.errstate(all="ignore"):
        q = F(1) / d
        a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
        ok = (d[a] >= near) & (d[b] >= near) & (d[c] >= near)
        area = _edge(u[a], v[a], u[b], v[b], u[c], v[c])
        ok &= (area != 0) & np.isfinite(area)
        i0 = np.maximum(F(0), np.floor(np.minimum(np.minimum(u[a], u[b]), u[c])))
        i1 = np.minimum(F(W - 1), np.floor(np.maximum(np.maximum(u[a], u[b]), u[c])))
        j0 = np.maximum(F(0), np.floor(np.minimum(np.minimum(v[a], v[b]), v[c])))
        j1 = np.minimum(F(H - 1), np.floor(np.maximum(np.maximum(v[a], v[b]), v[c])))
        ok &= (i0 <= i1) & (j0 <= j1)
    a, b, c, area, index = a[ok], b[ok], c[ok], area[ok], index[ok]
    i0, i1, j0, j1 = [t[ok].astype(np.int64) for t in (i0, i1, j0, j1)]
    ax, ay, bx, by, cx, cy, qa, qb, qc = u[a], v[a], u[b], v[b], u[c], v[c], q[a], q[b], q[c]
    bw, bh = i1 - i0 + 1, j1 - j0 + 1
    for dj in range(int(bh.max()) if len(bh) else 0):
        rows = np.nonzero(bh > dj)[0]
        for di in range(int(bw[rows].max())):
            k = rows[bw[rows] > di]
            i, j = i0[k] + di, j0[k] + dj
            px, py = i.astype(F) + F(0.5), j.astype(F) + F(0.5)
            with np.errstate(all="ignore"):
                wa = _edge(bx[k], by[k], cx[k], cy[k], px, py)
                wb = _edge(cx[k], cy[k], ax[k], ay[k], px, py)
                wc = _edge(ax[k], ay[k], bx[k], by[k], px, py)
                covered = np.where(area[k] > 0, (wa >= 0) & (wb >= 0) & (wc >= 0), (wa <= 0) & (wb <= 0) & (wc <= 0))
                z = area[k] / (wa * qa[k] + wb * qb[k] + wc * qc[k])
                covered &= (z > 0) & np.isfinite(z)
            key = (np.ascontiguousarray(z[covered], F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | index[k][covered].astype(np.uint64)
            np.minimum.at(kb, (j * W + i)[covered], key)
    return kb.reshape(H, W)


def key_buffers(vertices, faces, K, poses, img_wh, near):
    """(C, H, W) u64."""
    return np.stack([key_buffer(vertices, faces, K, p, img_wh, near) for p in np.asarray(poses, F)])


def sample(texture, T, n_faces, face, beta, gamma):
    """(n, 3) f32: the bilinear lookup of the rule at (beta, gamma) of each `face`; and the four texels it reads with their weights
    (i0, i1, j0, j1, fx, fy) for the tests of the tiling."""
    c, W, H = atlas_size(n_faces, T)
    face = np.asarray(face, np.int64)
    beta, gamma = np.asarray(beta, F), np.asarray(gamma, F)
    cell, slot1 = face >> 1, (face & 1) == 1
    ox, oy = ((cell % c) * (T + 5)).astype(F), ((cell // c) * (T + 4)).astype(F)
    xs, ys = F(1) + beta * F(T), F(1) + gamma * F(T)
    X = np.where(slot1, ox + (F(T + 4) - xs), ox + xs).astype(F)
    Y = np.where(slot1, oy + (F(T + 3) - ys), oy + ys).astype(F)
    flx, fly = np.floor(X), np.floor(Y)
    fx, fy = X - flx, Y - fly
    i0, j0 = flx.astype(np.int64), fly.astype(np.int64)
    i1, j1 = np.minimum(i0 + 1, W - 1), np.minimum(j0 + 1, H - 1)
    out = None
    if texture is not None:
        t = np.asarray(texture, np.uint8).reshape(H, W, 3).astype(F)
        fxc, fyc = fx[:, None], fy[:, None]
        top = t[j0, i0] * (F(1) - fxc) + t[j0, i1] * fxc
        bot = t[j1, i0] * (F(1) - fxc) + t[j1, i1] * fxc
        out = ((top * (F(1) - fyc) + bot * fyc) / F(255)).astype(F)
    return out, (i0, i1, j0, j1, fx, fy)


def render(vertices, faces, T, texture, K, poses, img_wh, near, background=(1, 1, 1), keys=None, return_weights=False):
    """image (C, H, W, 3) f32, face_index (C, H, W) i32, depth (C, H, W) f32 [, beta, gamma (C, H, W) f32, NaN where empty]."""
    W, H = img_wh
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    poses = np.asarray(poses, F)
    if keys is None:
        keys = key_buffers(vertices, faces, K, poses, img_wh, near)
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
        colour, _ = sample(texture, T, len(faces), f, beta, gamma)
        image[ci].reshape(-1, 3)[pix] = colour
        face_index[ci].reshape(-1)[pix] = f
        depth[ci].reshape(-1)[pix] = z
        betas[ci].reshape(-1)[pix], gammas[ci].reshape(-1)[pix] = beta, gamma
    return (image, face_index, depth, betas, gammas) if return_weights else (image, face_index, depth)


# ---- the shared scenes ------------------------------------------------------------------------------------------------------

def sphere_mesh(n, radius=0.7, jitter=0.2, seed=0):
    """Marching cubes (tests/mc_reference.py) of a sphere in the box [-1, 1]^3 at n^3, the vertices jittered by up to `jitter`
    voxel, and radial unit normals: vertices, faces, normals."""
    from tests import mc_reference as R
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, n, dtype=F)] * 3, indexing="ij")
    vol = (F(radius) - np.sqrt(x * x + y * y + z * z)).astype(F)
    v, f, _, _ = R.marching_cubes(vol, 0.0, (-1, -1, -1), (1, 1, 1))
    v = (v + np.random.RandomState(seed).uniform(-jitter, jitter, v.shape) * (2.0 / (n - 1))).astype(F)
    nrm = (v.astype(np.float64) / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True)).astype(F)
    return v, f, nrm


GRADIENT = np.array([[0.30, -0.20, 0.10], [-0.15, 0.25, 0.20], [0.10, 0.15, -0.30]])     # |G x| <= 0.43 on the sphere of radius 0.72


def linear_colour(points, dirs=None):
    """c(x) = 0.5 + G x in f32, one operation at a time (as the GPU test's torch color_fn computes it): inside [0.05, 0.95] for
    |x| <= 0.72."""
    p = np.asarray(points, F)
    g = GRADIENT.astype(F)
    return np.stack([F(0.5) + ((g[r, 0] * p[:, 0] + g[r, 1] * p[:, 1]) + g[r, 2] * p[:, 2]) for r in range(3)], 1)


def sphere_cameras(n, size, distance=2.0):
    """K (3, 3), poses (n, 3, 4), (W, H): n cameras at `distance` from the origin looking at it."""
    from tests.mesh_visibility_reference import intrinsics, look_at
    eyes = [(1, 0.3, 0.2), (-0.4, 1, 0.5), (0.2, -0.5, -1), (0, 0, 1), (-1, -1, 0.1)][:n]
    poses = np.stack([look_at(distance * np.asarray(e, np.float64) / np.linalg.norm(e), (0, 0, 0)) for e in eyes])
    return intrinsics(size * 1.2, size / 2.0, size / 2.0), poses, (size, size)
