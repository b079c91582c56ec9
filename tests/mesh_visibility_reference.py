"""Plain numpy float32 restatement of libngp_meshcull.so (include/ngp_meshcull.h, THE RULE), expression for expression: every
product and sum below is one f32 operation in the header's order (no `@`, no fused multiply-add), divisions are numpy's correctly
rounded f32 divisions.  `zbuffers`, `vertex_views`, `cull`; and the test scene the CPU and GPU tests share (two concentric shells,
cameras looking at them).  Test infrastructure only."""
import numpy as np

F = np.float32
INF_BITS = 0x7F800000


def camera_rows(pose):
    """The header's m (3, 3) = R^T and s (3,) = -(R^T t), summed left to right."""
    P = np.asarray(pose, F)
    m = np.ascontiguousarray(P[:3, :3].T)
    t = P[:3, 3]
    s = -(m[:, 0] * t[0] + m[:, 1] * t[1] + m[:, 2] * t[2])
    return m, s


def project(vertices, K, pose):
    """u, v, d (V,) f32 of every vertex in one camera."""
    x = np.asarray(vertices, F).reshape(-1, 3)
    K = np.asarray(K, F)
    m, s = camera_rows(pose)
    with np.errstate(all="ignore"):
        p = [m[r, 0] * x[:, 0] + m[r, 1] * x[:, 1] + m[r, 2] * x[:, 2] + s[r] for r in range(3)]
        ud, vd, d = [K[r, 0] * p[0] + K[r, 1] * p[1] + K[r, 2] * p[2] for r in range(3)]
        return ud / d, vd / d, d


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def zbuffer(vertices, faces, K, pose, img_wh, near):
    """(H, W) u32: the bits of the minimum depth per pixel of one camera, the bits of +inf where no face landed."""
    W, H = img_wh
    n_v = len(vertices)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    zb = np.full(H * W, INF_BITS, np.uint32)
    faces = faces[((faces >= 0) & (faces < n_v)).all(1)]
    if not len(faces):
        return zb.reshape(H, W)
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
    a, b, c, area = a[ok], b[ok], c[ok], area[ok]
    i0, i1, j0, j1 = [t[ok].astype(np.int64) for t in (i0, i1, j0, j1)]
    ax, ay, bx, by, cx, cy, qa, qb, qc = u[a], v[a], u[b], v[b], u[c], v[c], q[a], q[b], q[c]
    bw, bh = i1 - i0 + 1, j1 - j0 + 1
    # offset (di, dj) of every face's box at once: the faces whose box reaches that far
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
            np.minimum.at(zb, (j * W + i)[covered], np.ascontiguousarray(z[covered], F).view(np.uint32))
    return zb.reshape(H, W)


def zbuffers(vertices, faces, K, poses, img_wh, near):
    """(C, H, W) u32 depth bits."""
    return np.stack([zbuffer(vertices, faces, K, p, img_wh, near) for p in np.asarray(poses, F)])


def vertex_views(vertices, faces, K, poses, img_wh, bias, near, zbufs=None):
    """(V,) i32: the number of cameras in which each vertex has a view."""
    W, H = img_wh
    poses = np.asarray(poses, F)
    if zbufs is None:
        zbufs = zbuffers(vertices, faces, K, poses, img_wh, near)
    views = np.zeros(len(vertices), np.int32)
    near, bias = F(near), F(bias)
    for pose, zb in zip(poses, zbufs):
        u, v, d = project(vertices, K, pose)
        with np.errstate(all="ignore"):
            inside = (d >= near) & (u >= 0) & (u < F(W)) & (v >= 0) & (v < F(H))
            i = np.where(inside, np.floor(u), 0).astype(np.int64)
            j = np.where(inside, np.floor(v), 0).astype(np.int64)
            nearest = zb.reshape(H, W)[j, i].view(F)
            views += inside & (d <= nearest + bias)
    return views


def cull(vertices, faces, views, min_views, normals=None, colors=None):
    """-> vertices', faces', normals', colors': the faces in range with a vertex of at least min_views views and the vertices they
    reference, in the input's order, the faces re-indexed."""
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    n_v = len(vertices)
    in_range = ((faces >= 0) & (faces < n_v)).all(1)
    fkeep = in_range.copy()
    fkeep[in_range] = (np.asarray(views)[faces[in_range]] >= min_views).any(1)
    kept = faces[fkeep]
    used = np.zeros(n_v, bool)
    used[kept.reshape(-1)] = True
    remap = np.cumsum(used) - 1
    pick = lambda a: None if a is None else np.asarray(a)[used]
    return pick(vertices), remap[kept].astype(np.int32).reshape(-1, 3), pick(normals), pick(colors)


# ---- the shared scene -------------------------------------------------------------------------------------------------------

def shells_volume(shape=(40, 40, 40)):
    """(nz, ny, nx) f32 over the unit box: positive inside two concentric solid shells around (0.5, 0.5, 0.5), 0.30 < r < 0.40 and
    0.10 < r < 0.20; the iso-level 0 has four spherical sheets."""
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.linspace(0, 1, nz), np.linspace(0, 1, ny), np.linspace(0, 1, nx), indexing="ij")
    r = np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)
    return np.maximum(np.minimum(r - 0.30, 0.40 - r), np.minimum(r - 0.10, 0.20 - r)).astype(F)


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """(3, 4) f32 camera-to-world [R | t] of a camera at `eye` looking at `target`: columns right, down, forward (the camera looks
    along its +z, K's third row (0, 0, 1) makes d the forward distance)."""
    eye, target, up = [np.asarray(a, np.float64) for a in (eye, target, up)]
    fwd = (target - eye) / np.linalg.norm(target - eye)
    if abs(fwd @ up) > 0.9:
        up = np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    return np.concatenate([np.stack([right, down, fwd], 1), eye[:, None]], 1).astype(F)


def intrinsics(focal, cx, cy):
    return np.array([[focal, 0, cx], [0, focal, cy], [0, 0, 1]], F)


def ring_cameras(distance=1.5, centre=(0.5, 0.5, 0.5)):
    """14 poses at `distance` from `centre` along the 6 axis and the 8 diagonal directions, looking at it."""
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    dirs += [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
    c = np.asarray(centre, np.float64)
    return np.stack([look_at(c + distance * np.asarray(d, np.float64) / np.linalg.norm(d), c) for d in dirs])
