"""numpy restatement of THE RULE of ngp_pl_amd/csrc/meshchart/ngp_meshchart.h (libngp_meshchart.so): the snap to sixteenths of
a texel, the class of a face from its integer normal, charts as connected components, the shelves, texel owners, eviction over
three stages, dilation, texel points, UVs and the textured render.  Every decision is taken in integers, f32 and f64 expressions
are numpy's scalar-for-scalar, so the device must agree bit for bit, with no tolerance anywhere.  Also the test scenes.
"""
import numpy as np

from tests import mesh_atlas_reference as AR

F = np.float32
NO_CLASS = 6
NO_OWNER = 0xFFFFFFFF
MAX_WH = 16384
NEIGHBOURS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))


def snap_scale(s):
    return F(16.0 / float(F(s)))


def snap(vertices, faces, s):
    """face_class (F,) int64 and X (F, 3, 3) int64, the corners in sixteenths (zeros where the face has no class)."""
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    n_v, n_f = len(vertices), len(faces)
    cls = np.full(n_f, NO_CLASS, np.int64)
    X = np.zeros((n_f, 3, 3), np.int64)
    inr = ((faces >= 0) & (faces < n_v)).all(1)
    k = np.nonzero(inr)[0]
    if not len(k):
        return cls, X
    with np.errstate(all="ignore"):
        t = vertices[faces[k]] * snap_scale(s)                      # (n, 3, 3) f32
        fits = (np.abs(t) < F(4194304.0)).all((1, 2))
        Xi = np.rint(np.where(np.isfinite(t), t, F(0))).astype(np.int64)
    k, Xi = k[fits], Xi[fits]
    d1, d2 = Xi[:, 1] - Xi[:, 0], Xi[:, 2] - Xi[:, 0]
    n = np.stack([d1[:, 1] * d2[:, 2] - d1[:, 2] * d2[:, 1], d1[:, 2] * d2[:, 0] - d1[:, 0] * d2[:, 2],
                  d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]], 1)
    axis = np.argmax(np.abs(n), 1)                                  # the first maximum: the smallest axis on a tie
    nk = n[np.arange(len(k)), axis]
    good = nk != 0
    cls[k[good]] = 2 * axis[good] + (nk[good] < 0)
    X[k[good]] = Xi[good]
    return cls, X


def plane(cls, X):
    """(F, 3, 2) int64: the plane coordinates (u, v) of the corners; zeros where the face has no class."""
    out = np.zeros((len(cls), 3, 2), np.int64)
    for c in range(NO_CLASS):
        k = c >> 1
        a, b = (k + 1) % 3, (k + 2) % 3
        if c & 1:
            a, b = b, a
        m = cls == c
        out[m, :, 0], out[m, :, 1] = X[m][:, :, a], X[m][:, :, b]
    return out


def labels(faces, cls, active, unite=True):
    """(F,) int64: the smallest face index of the chart of every active face of a class, -1 for the others."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    act = np.asarray(active, bool) & (cls < NO_CLASS)
    parent = np.arange(len(faces))

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    if unite:
        edges = {}
        for f in np.nonzero(act)[0]:
            a, b, c = (int(x) for x in faces[f])
            for p, q in ((a, b), (b, c), (c, a)):
                edges.setdefault((min(p, q), max(p, q), int(cls[f])), []).append(int(f))
        for fs in edges.values():
            for g in fs[1:]:
                ra, rb = root(fs[0]), root(g)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    out = np.full(len(faces), -1, np.int64)
    for f in np.nonzero(act)[0]:
        out[f] = root(f)
    return out


def shelves(sizes, order, W, y0):
    x, y, shelf = 0, y0, 0
    origins = np.zeros((len(sizes), 2), np.int64)
    for i in order:
        w, h = int(sizes[i][0]), int(sizes[i][1])
        if x + w > W:
            y, x, shelf = y + shelf, 0, 0
        origins[i] = (x, y)
        x += w
        shelf = max(shelf, h)
    return origins, y + shelf


def pack(sizes, sort=True, width=0, y0=0):
    """origins (n, 2), order (n,), W, H so far of the rule's packing; ValueError when the atlas leaves 16384 texels."""
    sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
    n = len(sizes)
    order = sorted(range(n), key=lambda i: (-sizes[i][1], -sizes[i][0], i)) if sort else list(range(n))
    W = int(width)
    if W == 0:
        area = int((sizes[:, 0] * sizes[:, 1]).sum())
        r = int(np.sqrt(float(area)))
        while r * r < area:
            r += 1
        while r > 0 and (r - 1) * (r - 1) >= area:
            r -= 1
        W = max(int(sizes[:, 0].max()), r)
        while W <= MAX_WH and shelves(sizes, order, W, 0)[1] > W:
            W += max(1, W >> 4)
        if W > MAX_WH:
            raise ValueError("atlas wider than 16384")
    origins, H = shelves(sizes, order, W, y0)
    if H > MAX_WH:
        raise ValueError("atlas higher than 16384")
    return origins, np.asarray(order, np.int64), W, H


def _edge_in(px, py, qx, qy, Px, Py):
    dx, dy = qx - px, qy - py
    E = dx * (Py - py) - dy * (Px - px)
    return (E > 0) | ((E == 0) & ((dy > 0) | ((dy == 0) & (dx < 0))))


def covered(corners, W, H):
    """The flat indices of the texels of a W x H atlas whose centres the face with the atlas corners (3, 2) covers."""
    x, y = corners[:, 0], corners[:, 1]
    i0, i1 = max((int(x.min()) + 7) >> 4, 0), min((int(x.max()) - 8) >> 4, W - 1)
    j0, j1 = max((int(y.min()) + 7) >> 4, 0), min((int(y.max()) - 8) >> 4, H - 1)
    if i0 > i1 or j0 > j1:
        return np.zeros(0, np.int64)
    jj, ii = np.meshgrid(np.arange(j0, j1 + 1, dtype=np.int64), np.arange(i0, i1 + 1, dtype=np.int64), indexing="ij")
    Px, Py = 16 * ii + 8, 16 * jj + 8
    m = np.ones(ii.shape, bool)
    for p, q in ((0, 1), (1, 2), (2, 0)):
        m &= _edge_in(int(x[p]), int(y[p]), int(x[q]), int(y[q]), Px, Py)
    return (jj[m] * W + ii[m]).reshape(-1)


def dilate(owner, pad):
    """pad passes of the rule's dilation over owner (H, W) int64 with NO_OWNER where unowned."""
    H, W = owner.shape
    for _ in range(pad):
        src, out = owner, owner.copy()
        for dx, dy in reversed(NEIGHBOURS):                         # backwards: the first owned neighbour of the order is kept
            nb = np.full((H, W), NO_OWNER, np.int64)
            ys, yd = (slice(1, H), slice(0, H - 1)) if dy > 0 else ((slice(0, H - 1), slice(1, H)) if dy < 0 else (slice(0, H), slice(0, H)))
            xs, xd = (slice(1, W), slice(0, W - 1)) if dx > 0 else ((slice(0, W - 1), slice(1, W)) if dx < 0 else (slice(0, W), slice(0, W)))
            nb[yd, xd] = src[ys, xs]
            take = (src == NO_OWNER) & (nb != NO_OWNER)
            out[take] = nb[take]
        owner = out
    return owner


class Charts:
    """Everything the restatement derives from a mesh, texel_size s and pad, computed once."""

    def __init__(self, vertices, faces, s, pad=2):
        vertices = np.asarray(vertices, F).reshape(-1, 3)
        faces = np.asarray(faces, np.int64).reshape(-1, 3)
        n_f = len(faces)
        self.s, self.pad = float(F(s)), int(pad)
        self.face_class, self.X = snap(vertices, faces, s)
        uv = plane(self.face_class, self.X)
        self.face_chart = np.full(n_f, -1, np.int64)
        self.labels, self.charts_per_stage, self.evicted_per_stage = [], [], []
        self.corner_texels = np.zeros((n_f, 3, 2), np.int64)
        rects = []
        W = H = 0
        owner = np.zeros((0, 0), np.int64)
        active = self.face_class < NO_CLASS
        if not active.any():
            raise ValueError("no face has a chart")
        for stage in range(3):
            if not active.any():
                break
            lab = labels(faces, self.face_class, active, unite=stage < 2)
            self.labels.append(lab)
            roots = np.unique(lab[lab >= 0])
            base = len(rects)
            members = np.nonzero(lab >= 0)[0]
            self.face_chart[members] = base + np.searchsorted(roots, lab[members])
            sizes, origin = [], []
            for c in range(len(roots)):
                pts = uv[self.face_chart == base + c].reshape(-1, 2)
                o = pts.min(0) >> 4
                wh = (pts.max(0) >> 4) - o + 1
                sizes.append(wh + 2 * self.pad)
                origin.append(o)
            org, _, W, H = pack(sizes, sort=stage < 2, width=W, y0=H)
            for c in range(len(roots)):
                rects.append((org[c][0], org[c][1], sizes[c][0], sizes[c][1], origin[c][0], origin[c][1]))
            grown = np.full((H, W), NO_OWNER, np.int64)
            if owner.size:
                grown[:owner.shape[0]] = owner
            owner = grown
            flat = owner.reshape(-1)
            for f in members:
                r = rects[self.face_chart[f]]
                self.corner_texels[f] = uv[f] + 16 * np.asarray([r[0] + self.pad - r[4], r[1] + self.pad - r[5]], np.int64)
            cover = {int(f): covered(self.corner_texels[f], W, H) for f in members}
            for f in members:                                       # the smallest covering face: ascending, first come
                t = cover[int(f)]
                t = t[flat[t] == NO_OWNER]
                flat[t] = f
            self.charts_per_stage.append(len(roots))
            evicted = np.zeros(n_f, bool)
            if stage < 2:
                for f in members:
                    evicted[f] = bool((flat[cover[int(f)]] != f).any())
                flat[(flat != NO_OWNER) & evicted[np.where(flat != NO_OWNER, flat, 0)]] = NO_OWNER
                self.evicted_per_stage.append(int(evicted.sum()))
            active = evicted
        self.W, self.H = W, H
        self.n_charts = len(rects)
        self.chart_rects = np.asarray(rects, np.int64).reshape(-1, 6)
        self.owner = owner
        tf = dilate(owner, self.pad)
        self.texel_face = np.where(tf == NO_OWNER, -1, tf).astype(np.int32)
        ct = self.corner_texels.astype(np.float64)
        self.uvs = np.stack([(ct[..., 0] / 16.0) / float(W), 1.0 - (ct[..., 1] / 16.0) / float(H)], -1).astype(F)


def _edge_fn(px, py, qx, qy, Px, Py):
    return (qx - px) * (Py - py) - (qy - py) * (Px - px)


def texel_points(vertices, faces, normals, charts, box, begin=0, count=None):
    """points (n, 3) f32, dirs (n, 3) f32, valid (n,) u8 of the texels begin .. begin+count-1."""
    vertices, normals = np.asarray(vertices, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    box = np.asarray(box, F).reshape(6)
    total = charts.W * charts.H
    count = total - begin if count is None else count
    g = np.arange(begin, begin + count, dtype=np.int64)
    face = charts.texel_face.reshape(-1)[g].astype(np.int64)
    n = len(g)
    points = np.tile(box[:3], (n, 1)).astype(F)
    dirs = np.tile(F([0, 0, 1]), (n, 1))
    valid = np.zeros(n, np.uint8)
    ok = (face >= 0) & (face < len(faces))
    ok &= ((faces[np.where(ok, face, 0)] >= 0) & (faces[np.where(ok, face, 0)] < len(vertices))).all(1)
    c0 = charts.corner_texels[np.where(ok, face, 0)]
    ok &= _edge_fn(c0[:, 0, 0], c0[:, 0, 1], c0[:, 1, 0], c0[:, 1, 1], c0[:, 2, 0], c0[:, 2, 1]) > 0
    k = np.nonzero(ok)[0]
    if not len(k):
        return points, dirs, valid
    f = face[k]
    ct = charts.corner_texels[f]
    Px, Py = 16 * (g[k] % charts.W) + 8, 16 * (g[k] // charts.W) + 8
    ax, ay, bx, by, cx, cy = ct[:, 0, 0], ct[:, 0, 1], ct[:, 1, 0], ct[:, 1, 1], ct[:, 2, 0], ct[:, 2, 1]
    area = _edge_fn(ax, ay, bx, by, cx, cy).astype(np.float64)
    u = (_edge_fn(cx, cy, ax, ay, Px, Py).astype(np.float64) / area).astype(F)[:, None]
    v = (_edge_fn(ax, ay, bx, by, Px, Py).astype(np.float64) / area).astype(F)[:, None]
    a, b, c = [faces[f, m] for m in range(3)]
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


def sample(texture, corner_texels, face, beta, gamma):
    """(n, 3) f32: the rule's bilinear lookup at (beta, gamma) of each `face`."""
    texture = np.asarray(texture, np.uint8)
    H, W = texture.shape[:2]
    t = texture.astype(F)
    with np.errstate(all="ignore"):
        c = np.asarray(corner_texels)[face].astype(F) / F(16)
        beta, gamma = np.asarray(beta, F), np.asarray(gamma, F)
        X = ((c[:, 0, 0] + beta * (c[:, 1, 0] - c[:, 0, 0])) + gamma * (c[:, 2, 0] - c[:, 0, 0])) - F(0.5)
        Y = ((c[:, 0, 1] + beta * (c[:, 1, 1] - c[:, 0, 1])) + gamma * (c[:, 2, 1] - c[:, 0, 1])) - F(0.5)
        flx, fly = np.floor(X), np.floor(Y)
        fx, fy = (X - flx)[:, None], (Y - fly)[:, None]
        i0 = np.minimum(np.maximum(np.clip(flx, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64), 0), W - 1)
        j0 = np.minimum(np.maximum(np.clip(fly, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64), 0), H - 1)
        i1, j1 = np.minimum(i0 + 1, W - 1), np.minimum(j0 + 1, H - 1)
        top = t[j0, i0] * (F(1) - fx) + t[j0, i1] * fx
        bot = t[j1, i0] * (F(1) - fx) + t[j1, i1] * fx
        return ((top * (F(1) - fy) + bot * fy) / F(255)).astype(F)


def render(vertices, faces, corner_texels, texture, K, poses, img_wh, near, background=(1, 1, 1)):
    """image (C, H, W, 3) f32, face_index (C, H, W) i32, depth (C, H, W) f32: the shared rasteriser's winners and weights (the
    restatement of csrc/meshatlas/ngp_meshatlas.h), shaded by this rule."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    dummy = np.zeros((len(faces), 2), np.int32)
    blank = np.zeros((1, 1, 3), np.uint8)
    _, face_index, depth, beta, gamma = AR.render(vertices, faces, dummy, blank, K, poses, img_wh, near, background, return_weights=True)
    image = np.empty(face_index.shape + (3,), F)
    image[:] = np.asarray(background, F)
    m = face_index >= 0
    image[m] = sample(texture, corner_texels, face_index[m].astype(np.int64), beta[m], gamma[m])
    return image, face_index, depth


# ---- scenes ----------------------------------------------------------------------------------------------------------------------

def sheet(n_faces, seed=0, radius=0.3, width=0.5):
    """A jittered grid bent over half a cylinder (so that charts of several classes meet), cut to exactly n_faces faces."""
    rng = np.random.default_rng(seed)
    ny = max(1, int(np.sqrt(n_faces / 2.0)))
    nx = (n_faces + 2 * ny - 1) // (2 * ny)
    th = np.linspace(0.1, np.pi - 0.1, nx + 1)
    vy = np.linspace(-width / 2, width / 2, ny + 1)
    T, Y = np.meshgrid(th, vy, indexing="ij")
    v = np.stack([radius * np.cos(T), Y, radius * np.sin(T)], -1).reshape(-1, 3)
    v += rng.uniform(-0.2, 0.2, v.shape) * min(radius * (np.pi - 0.2) / nx, width / ny)
    idx = np.arange((nx + 1) * (ny + 1)).reshape(nx + 1, ny + 1)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
    f = np.stack([np.stack([a, b, d], -1), np.stack([a, d, c], -1)], 2).reshape(-1, 3)
    return v.astype(F), f[:n_faces].astype(np.int32)


def box12(half=0.3):
    """A box of 12 faces, normals outwards."""
    v = np.asarray([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], F)
    f = np.asarray([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                    [1, 5, 7], [1, 7, 3]], np.int32)
    return v, f


def helicoid(turns=3, segments=24, r0=0.15, r1=0.4, pitch=0.2):
    """A ramp that winds over itself: its projection on the xy plane overlaps `turns` times."""
    n = turns * segments
    t = 2.0 * np.pi * np.arange(n + 1) / segments
    z = pitch * np.arange(n + 1) / segments - pitch * turns / 2.0
    inner = np.stack([r0 * np.cos(t), r0 * np.sin(t), z], 1)
    outer = np.stack([r1 * np.cos(t), r1 * np.sin(t), z], 1)
    v = np.concatenate([inner, outer]).astype(F)
    f = []
    for i in range(n):
        a, b, c, d = i, n + 1 + i, i + 1, n + 1 + i + 1               # inner, outer of this step; inner, outer of the next
        f += [(a, c, d), (a, d, b)]
    return v, np.asarray(f, np.int32)


def book():
    """Three faces on one edge (a non-manifold edge), two of them in one plane class, and a fourth face on one page."""
    v = np.asarray([[0, 0, 0], [0, 0.3, 0], [0.3, 0.1, 0.02], [-0.3, 0.15, 0.03], [0.02, 0.1, 0.3], [0.32, 0.4, 0.0]], F)
    f = np.asarray([[0, 1, 3], [1, 0, 2], [0, 1, 4], [1, 2, 5]], np.int32)
    return v, f


def affine_colour(p, d=None):
    """A colour that is affine in the point: bilinear blends across a flat chart are exact."""
    p = np.asarray(p, np.float64)
    return np.stack([0.5 + 0.6 * p[:, 0], 0.5 + 0.6 * p[:, 1], 0.5 + 0.6 * p[:, 2]], 1)
