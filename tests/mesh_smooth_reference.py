"""Plain numpy restatement of libngp_meshsmooth.so (include/ngp_meshsmooth.h, THE RULE), written from the rule: float32 where the
rule says f32, int64 states and sums, float64 for the steps and the normals with one rounding to float32 at the end; np.unique
where the library hashes, np.add.at where it gathers or adds atomically.  Test infrastructure only."""
import numpy as np

Q = 1 << 16
QMAX = 1 << 30
NQ = 1 << 20
INSIDE, BOUNDARY, FREE = 1, 2, 4


def states(vertices, origin, cell):
    """inside (V,) bool, q (V, 3) int64 (0 where outside)."""
    x = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    o = np.asarray(origin, np.float32).reshape(3)
    with np.errstate(all="ignore"):
        t = (x - o[None, :]) / np.float32(cell)
        r = np.rint(t * np.float32(Q))
        inside = (np.isfinite(t) & (np.abs(r) <= np.float32(QMAX))).all(1)
    assert t.dtype == r.dtype == np.float32
    q = np.where(inside[:, None], r, np.float32(0)).astype(np.int64)
    return inside, q


def edges(faces, inside):
    """The distinct edges (E, 2) int64 with a < b, ascending, and how often each occurs (E,) int64."""
    n_v = len(inside)
    f = np.asarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    valid = ((f >= 0) & (f < n_v)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    f = f[valid]
    sides = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    sides = sides[inside[sides[:, 0]] & inside[sides[:, 1]]]
    keys = np.minimum(sides[:, 0], sides[:, 1]) << 32 | np.maximum(sides[:, 0], sides[:, 1])
    assert keys.dtype == np.int64
    keys, occurrences = np.unique(keys, return_counts=True)
    return np.stack([keys >> 32, keys & 0xFFFFFFFF], 1).reshape(-1, 2), occurrences.astype(np.int64)


def topology(vertices, faces, origin, cell, pin_boundary=True):
    """degree (V,) int32, flags (V,) uint8, totals (4,) int64 = edges, boundary edges, free vertices, boundary vertices; and the
    edges (E, 2) int64."""
    inside, _ = states(vertices, origin, cell)
    n_v = len(inside)
    e, occurrences = edges(faces, inside)
    degree = np.zeros(n_v, np.int64)
    np.add.at(degree, e[:, 0], 1)
    np.add.at(degree, e[:, 1], 1)
    boundary = np.zeros(n_v, bool)
    boundary[e[occurrences == 1].reshape(-1)] = True
    free = inside & (degree > 0) & ~(boundary & bool(pin_boundary))
    flags = (inside * INSIDE + boundary * BOUNDARY + free * FREE).astype(np.uint8)
    totals = np.array([len(e), (occurrences == 1).sum(), free.sum(), boundary.sum()], np.int64)
    return degree.astype(np.int32), flags, totals, e


def one_pass(q, e, degree, free, factor, trace=None):
    """The states after a pass with `factor` (a float32); trace, a dict, counts the exact halves rint met and the clamped values."""
    assert q.dtype == np.int64
    f = np.float64(np.float32(factor))
    total = np.zeros_like(q)
    np.add.at(total, e[:, 0], q[e[:, 1]])
    np.add.at(total, e[:, 1], q[e[:, 0]])
    d = degree.astype(np.int64)[free]
    D = total[free] - d[:, None] * q[free]
    assert D.dtype == np.int64 and np.abs(D).max(initial=0) < 1 << 62
    x = f * (D.astype(np.float64) / d.astype(np.float64)[:, None])
    assert x.dtype == np.float64
    moved = q[free] + np.rint(x).astype(np.int64)
    out = q.copy()
    out[free] = np.minimum(np.maximum(moved, -QMAX), QMAX)
    if trace is not None:
        trace["ties"] = trace.get("ties", 0) + int((np.abs(x - np.trunc(x)) == 0.5).sum())
        trace["clamped"] = trace.get("clamped", 0) + int((moved != out[free]).sum())
        trace["at_qmax"] = trace.get("at_qmax", 0) + int((np.abs(out[free]) == QMAX).sum())
    return out


def taubin(vertices, faces, origin, cell, pairs, lam, mu, pin_boundary=True, trace=None):
    """vertices' (V, 3) float32 after `pairs` pairs of passes (lam, then mu)."""
    vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    _, q = states(vertices, origin, cell)
    degree, flags, _, e = topology(vertices, faces, origin, cell, pin_boundary)
    free = (flags & FREE) != 0
    for _ in range(int(pairs)):
        q = one_pass(q, e, degree, free, lam, trace)
        q = one_pass(q, e, degree, free, mu, trace)
    o = np.asarray(origin, np.float32).reshape(3).astype(np.float64)
    moved = (o[None, :] + (q.astype(np.float64) / np.float64(Q)) * np.float64(np.float32(cell))).astype(np.float32)
    out = vertices.copy()
    out[free] = moved[free]
    return out


def normals(vertices, faces):
    """(V, 3) float32 geometric normals."""
    x = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    n_v = len(x)
    f = np.asarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    f = f[((f >= 0) & (f < n_v)).all(1)]
    a, b, c = x[f[:, 0]], x[f[:, 1]], x[f[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
        length = np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
        unit = cr / length[:, None]
        ok = (length > 0) & np.isfinite(unit).all(1)
        add = np.rint(unit[ok] * np.float64(NQ))
    assert unit.dtype == add.dtype == np.float64
    add = add.astype(np.int64)
    N = np.zeros((n_v, 3), np.int64)
    for k in range(3):
        np.add.at(N, f[ok][:, k], add)
    assert np.abs(N).max(initial=0) < 1 << 51
    N = N.astype(np.float64)
    length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(length == 0, np.float64(0), N / length).astype(np.float32)
