"""Plain numpy restatement of libngp_meshsimplify.so (include/ngp_meshsimplify.h, THE RULE), written from the rule: float32 where
the rule says f32, int64 sums, float64 for the means with one rounding to float32 at the end; np.unique and dictionaries where
the library hashes.  Test infrastructure only."""
import numpy as np

Q = 1 << 20
CELLS = 1 << 21


def cells(vertices, origin, cell):
    """inside (V,) bool, c (V, 3) int64 (0 where outside), key (V,) int64, q (V, 3) int64."""
    x = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    o = np.asarray(origin, np.float32).reshape(3)
    with np.errstate(all="ignore"):
        t = (x - o[None, :]) / np.float32(cell)
        fl = np.floor(t)
        inside = (np.isfinite(t) & (fl >= 0) & (fl < np.float32(CELLS))).all(1)
        c = np.where(inside[:, None], fl, np.float32(0)).astype(np.int64)
        frac = t - c.astype(np.float32)
        q = np.rint(frac * np.float32(Q))
    assert t.dtype == fl.dtype == frac.dtype == q.dtype == np.float32
    q = np.where(inside[:, None], q, np.float32(0)).astype(np.int64)
    key = c[:, 0] | c[:, 1] << 21 | c[:, 2] << 42
    return inside, c, key, q


def vertex_labels(vertices, origin, cell):
    """(V,) int32: the smallest vertex index with the vertex's key, -1 outside the grid."""
    inside, _, key, _ = cells(vertices, origin, cell)
    label = np.full(len(key), -1, np.int32)
    first = {}
    for v in np.nonzero(inside)[0].tolist():
        label[v] = first.setdefault(int(key[v]), v)
    return label


def _fixed(a, lo):
    a = np.asarray(a, np.float32)
    with np.errstate(invalid="ignore"):
        r = np.rint(np.minimum(np.maximum(a, np.float32(lo)), np.float32(1)) * np.float32(Q))
    assert r.dtype == np.float32
    return np.where(np.isnan(a), np.float32(0), r).astype(np.int64)


def _sum_by(label, members, values, size):
    out = np.zeros((size, 3), np.int64)
    np.add.at(out, label[members], values[members])
    return out


def simplify(vertices, faces, origin, cell, normals=None, colors=None):
    """-> vertices' (V', 3) f32, faces' (F', 3) i32, normals', colors' (None stays None), label (V,) i32, clusters."""
    vertices = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    n_v = len(vertices)
    inside, c, _, q = cells(vertices, origin, cell)
    label = vertex_labels(vertices, origin, cell)
    members = np.nonzero(inside)[0]
    clusters = int((label == np.arange(n_v)).sum())
    # faces: indices in range, labels >= 0 and pairwise different; the first of every set of labels is kept
    f64 = faces.astype(np.int64)
    in_range = ((f64 >= 0) & (f64 < n_v)).all(1)
    lab = np.full(faces.shape, -1, np.int64)
    lab[in_range] = label[f64[in_range]]
    survives = in_range & (lab >= 0).all(1) & (lab[:, 0] != lab[:, 1]) & (lab[:, 1] != lab[:, 2]) & (lab[:, 0] != lab[:, 2])
    seen, kept = set(), []
    for f in np.nonzero(survives)[0].tolist():
        s = tuple(sorted(lab[f].tolist()))
        if s not in seen:
            seen.add(s)
            kept.append(f)
    kept_labels = lab[kept].reshape(-1, 3)
    out_labels = np.unique(kept_labels)                                        # ascending
    faces_out = np.searchsorted(out_labels, kept_labels).astype(np.int32).reshape(-1, 3)
    # attributes: int64 sums over every member, referenced by a face or not
    n = np.bincount(label[members], minlength=n_v).astype(np.int64)[out_labels].astype(np.float64)[:, None]
    o = np.asarray(origin, np.float32).reshape(3).astype(np.float64)
    P = _sum_by(label, members, q, n_v)[out_labels]
    assert np.abs(P).max(initial=0) < 1 << 51
    pos = (o[None, :] + (c[out_labels].astype(np.float64) + (P.astype(np.float64) / n) / np.float64(Q)) * np.float64(np.float32(cell))).astype(np.float32)
    nrm = col = None
    if normals is not None:
        N = _sum_by(label, members, _fixed(np.asarray(normals, np.float32).reshape(-1, 3), -1.0), n_v)[out_labels].astype(np.float64)
        length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])[:, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            nrm = np.where(length == 0, np.float64(0), N / length).astype(np.float32)
    if colors is not None:
        C = _sum_by(label, members, _fixed(np.asarray(colors, np.float32).reshape(-1, 3), 0.0), n_v)[out_labels].astype(np.float64)
        col = ((C / n) / np.float64(Q)).astype(np.float32)
    return pos.reshape(-1, 3), faces_out, nrm, col, label, clusters
