"""numpy restatement of include/ngp_meshdecimate.h, round by round and vectorised over the pairs (target, corner) of every removable
vertex: begin, evaluate (REMOVABLE, VALID, COST, KEY, WINNERS), apply, output, and the caller's loop of the header as `decimate`.
Face and edge sets are int64 keys: n_vertices^3 must stay below 2^63 (two million vertices), which is a limit of this file only."""
import numpy as np

MAX_DEGREE = 64
S = 2.0 ** 20
CAP = 2.0 ** 50
NONE = np.uint64(2 ** 64 - 1)


def mix(u):
    x = np.asarray(u).astype(np.uint32)
    with np.errstate(over="ignore"):
        x = x * np.uint32(0x9E3779B1)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x85EBCA77)
        x = x ^ (x >> np.uint32(13))
    return x


def code(c):
    """The header's code(): a cost to 24 significant bits, truncated, as uint64."""
    c = np.asarray(c, np.int64)
    x, e = c.copy(), np.zeros(c.shape, np.int64)                               # e: the highest set bit
    for s in (32, 16, 8, 4, 2, 1):
        m = (x >> s) != 0
        e += np.where(m, s, 0)
        x = np.where(m, x >> s, x)
    m = np.where(e >= 23, c >> np.maximum(e - 23, 0), c << np.maximum(23 - e, 0))
    return np.where(c > 0, ((e + 1) << 23) | (m & 0x7FFFFF), 0).astype(np.uint64)


def begin(faces, n_v):
    """The current faces (F, 3) int64: a face with an index out of range or repeated is dead, (-1, -1, -1)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3).copy()
    ok = ((f >= 0) & (f < n_v)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    f[~ok] = -1
    return f


def _cross(p, q):
    return np.stack([p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]], -1)


def _dot(p, q):
    return (p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]


def corners(cur, n_v):
    """The corners (u, a, b) of the current faces grouped by u, the degrees and the rows' starts."""
    f = cur[cur[:, 0] >= 0]
    cu, ca, cb = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1), f[:, [2, 0, 1]].reshape(-1)
    order = np.argsort(cu, kind="stable")
    cu, ca, cb = cu[order], ca[order], cb[order]
    deg = np.bincount(cu, minlength=n_v)
    return f, cu, ca, cb, deg, np.cumsum(deg) - deg


def removable(vertices, cu, ca, cb, deg, start):
    """(V,) bool: REMOVABLE of the header."""
    n_v = len(vertices)
    finite = np.isfinite(vertices).all(1)
    ok = (deg >= 3) & (deg <= MAX_DEGREE) & finite
    if len(cu) == 0:
        return ok
    ka, kb = cu * n_v + ca, cu * n_v + cb
    ua, na = np.unique(ka, return_counts=True)
    ub, nb = np.unique(kb, return_counts=True)
    found = np.minimum(np.searchsorted(ua, kb), len(ua) - 1)
    bad = (na[np.searchsorted(ua, ka)] != 1) | (nb[np.searchsorted(ub, kb)] != 1) | (ua[found] != kb) | ~finite[ca]
    ok &= np.bincount(cu[bad], minlength=n_v) == 0
    by_a = np.argsort(ka, kind="stable")
    succ = by_a[np.minimum(np.searchsorted(ka[by_a], kb), len(ka) - 1)]        # meaningful at the corners of vertices still ok
    us = np.nonzero(ok)[0]
    if len(us):
        at, first = start[us].copy(), np.zeros(len(us), np.int64)
        for step in range(1, int(deg[us].max()) + 1):
            at = succ[at]
            first[(at == start[us]) & (first == 0)] = step
        ok[us] = first == deg[us]
    return ok


def evaluate(vertices, cur, cell, max_error=None):
    """One round up to WINNERS: key (V,) uint64 (NONE for no candidate), target (V,) int64, won (V,) bool, totals
    (candidates, winners, current faces)."""
    vertices = np.asarray(vertices, np.float32)
    n_v = len(vertices)
    x = vertices.astype(np.float64)
    f, cu, ca, cb, deg, start = corners(cur, n_v)
    key, target = np.full(n_v, NONE, np.uint64), np.full(n_v, -1, np.int64)
    rem = removable(vertices, cu, ca, cb, deg, start)
    c64 = np.float64(np.float32(cell))
    kc, kl = S / ((c64 * c64) * c64), S / (c64 * c64)
    e2 = None if max_error is None or max_error < 0 else np.float64(np.float32(max_error)) * np.float64(np.float32(max_error))
    if rem.any():
        lo, hi = np.minimum(f, f[:, [1, 2, 0]]), np.maximum(f, f[:, [1, 2, 0]])
        ekeys = np.unique(lo * n_v + hi)
        fs = np.sort(f, 1)
        fkeys = np.unique((fs[:, 0] * n_v + fs[:, 1]) * n_v + fs[:, 2])
    with np.errstate(all="ignore"):
        for d in np.unique(deg[rem]):
            ud = np.nonzero(rem & (deg == d))[0]
            idx = start[ud][:, None] + np.arange(d)[None, :]
            A, B = ca[idx], cb[idx]                                                # (n, d)
            pu, pa, pb = x[ud], x[A], x[B]
            c = _cross(pa - pu[:, None], pb - pu[:, None])                         # (n, k, 3)
            ll = _dot(c, c)
            L = np.sqrt(ll)
            V, Ak, Bk = A[:, :, None], A[:, None, :], B[:, None, :]                # targets along axis 1, corners along axis 2
            pv = pa[:, :, None, :]
            dv = pa - pu[:, None]                                                  # (n, i, 3)
            q = _cross(pa[:, None] - pv, pb[:, None] - pv)                         # (n, i, k, 3)
            ck = c[:, None]
            dot = _dot(ck, q)
            g = _dot(ck, dv[:, :, None, :])
            ok = dot > 0
            if e2 is not None:
                ok &= g * g <= e2 * ll[:, None, :]
            linked = (Ak != V) & np.isin(np.minimum(V, Ak) * n_v + np.maximum(V, Ak), ekeys)
            tri = np.sort(np.stack(np.broadcast_arrays(V, Ak, Bk), -1), -1)
            dup = np.isin((tri[..., 0] * n_v + tri[..., 1]) * n_v + tri[..., 2], fkeys)
            judged = (Ak != V) & (Bk != V)
            valid = (linked.sum(2) == 2) & ~(judged & (~ok | dup)).any(2)
            term = np.where(judged & ok, np.fmin(((g * g) / L[:, None, :]) * kc, CAP), 0.0)
            cost = np.rint(term).astype(np.int64).sum(2)
            vlen = np.rint(np.fmin(_dot(dv, dv) * kl, CAP)).astype(np.int64)
            best = np.lexsort((A, vlen, cost, ~valid), axis=1)[:, 0]
            rows = np.arange(len(ud))
            has = valid[rows, best]
            target[ud[has]] = A[rows, best][has]
            key[ud[has]] = (code(cost[rows, best][has]) << np.uint64(32)) | mix(ud[has]).astype(np.uint64)
    cand = key != NONE
    claim = np.full(n_v, NONE, np.uint64)
    np.minimum.at(claim, np.nonzero(cand)[0], key[cand])
    ring = cand[cu] if len(cu) else np.zeros(0, bool)
    np.minimum.at(claim, ca[ring], key[cu[ring]])
    lost = claim[ca[ring]] != key[cu[ring]]
    won = cand & (claim == key) & (np.bincount(cu[ring][lost], minlength=n_v) == 0)
    return key, target, won, (int(cand.sum()), int(won.sum()), len(f))


def apply(cur, key, target, won, n_keep):
    """APPLY: the n_keep winners with the smallest keys; returns the new current faces and the applied vertices."""
    w = np.nonzero(won)[0]
    w = w[np.argsort(key[w], kind="stable")][:n_keep]
    to = np.arange(len(key) + 1)                                               # the spare last entry takes the dead faces' -1
    to[w] = target[w]
    to[-1] = -1
    out = to[cur]
    live = out[:, 0] >= 0
    out[live & ((out[:, 0] == out[:, 1]) | (out[:, 1] == out[:, 2]) | (out[:, 0] == out[:, 2]))] = -1
    return out, w


def output(vertices, cur, normals=None, colors=None):
    f = cur[cur[:, 0] >= 0]
    used = np.unique(f)
    remap = np.full(len(vertices) + 1, -1, np.int64)
    remap[used] = np.arange(len(used))
    pick = lambda a: None if a is None else np.asarray(a, np.float32)[used]
    return pick(vertices), remap[f].astype(np.int32).reshape(-1, 3), pick(normals), pick(colors)


def decimate(vertices, faces, cell, target_faces=None, max_error=None, normals=None, colors=None, trace=None):
    """The caller's loop of the header -> vertices, faces, normals, colours, stats.  stats: rounds (those that applied a collapse),
    totals (R, 4) int64 per evaluated round: candidates, winners, current faces, applied; reached; faces.  target_faces >= F
    returns the input.  trace(cur, applied vertices) is called after every apply."""
    assert target_faces is not None or max_error is not None
    vertices = np.asarray(vertices, np.float32)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    totals = []
    if target_faces is not None and target_faces >= len(faces):
        return vertices, faces, normals, colors, dict(rounds=0, totals=np.zeros((0, 4), np.int64), reached=True, faces=len(faces))
    cur = begin(faces, len(vertices))
    n_f = None
    while n_f is None or target_faces is None or n_f > target_faces:
        key, target, won, (n_c, n_w, n_f) = evaluate(vertices, cur, cell, max_error)
        if (target_faces is not None and n_f <= target_faces) or n_c == 0:
            totals.append([n_c, n_w, n_f, 0])
            break
        n_keep = n_w if target_faces is None else min(n_w, (n_f - target_faces + 1) // 2)
        cur, applied = apply(cur, key, target, won, n_keep)
        if trace is not None:
            trace(cur, applied)
        totals.append([n_c, n_w, n_f, n_keep])
        n_f -= 2 * n_keep
    totals = np.array(totals, np.int64).reshape(-1, 4)
    v, f, n, c = output(vertices, cur, normals, colors)
    assert len(f) == n_f
    return v, f, n, c, dict(rounds=int((totals[:, 3] > 0).sum()), totals=totals, reached=target_faces is None or n_f <= target_faces,
                            faces=n_f)
