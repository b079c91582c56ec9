"""Plain numpy restatement of libngp_meshquadric.so (include/ngp_meshquadric.h, THE RULE), line by line: float32 where the rule
says f32, float64 one operation at a time where it says f64 (numpy never fuses a multiply and an add), int64 sums with np.add.at
where the library adds atomically, the 3x3 solve written out (no np.linalg).  Cells, fractions and labels are those of
tests/mesh_simplify_reference.py.  Test infrastructure only."""
import numpy as np

from tests import mesh_simplify_reference as SR

Q = 1 << 20
S = np.float64(1 << 24)
W_MAX = np.float64(16)
EPS = np.float64(2.0 ** -10)
SUMS = 14
NOT_LEADER, QUADRIC, MEAN_NO_FACES, MEAN_OUTSIDE = 0, 1, 2, 3


def _rint64(x):
    return np.rint(x).astype(np.int64)


def sums(vertices, faces, label, origin, cell):
    """(V, 14) int64, indexed by label: n, P[3], A00 A01 A02 A11 A12 A22, B[3], Wsum.  Rows that are no label stay 0."""
    x32 = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int32).reshape(-1, 3).astype(np.int64)
    label = np.asarray(label, np.int32).astype(np.int64)
    n_v = len(x32)
    out = np.zeros((n_v, SUMS), np.int64)
    inside, _, _, q = SR.cells(x32, origin, cell)
    # member sums
    member = inside & (label >= 0) & (label < n_v)
    mv = np.nonzero(member)[0]
    np.add.at(out[:, 0], label[mv], 1)
    np.add.at(out[:, 1:4], label[mv], q[mv])
    # corner sums
    x = x32.astype(np.float64)
    y_all = q.astype(np.float64) / np.float64(Q) - np.float64(0.5)
    cell2 = np.float64(np.float32(cell)) * np.float64(np.float32(cell))
    in_range = ((faces >= 0) & (faces < n_v)).all(1)
    for j in range(3):
        a, b, c = faces[in_range, j], faces[in_range, (j + 1) % 3], faces[in_range, (j + 2) % 3]
        keep = member[a]
        a, b, c = a[keep], b[keep], c[keep]
        with np.errstate(all="ignore"):
            e1, e2 = x[b] - x[a], x[c] - x[a]
            cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                           e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                           e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
            L = np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
            ok = np.isfinite(L) & (L > 0)
        a, cr, L = a[ok], cr[ok], L[ok]
        n = cr / L[:, None]
        with np.errstate(over="ignore"):
            w = np.minimum((np.float64(0.5) * L) / cell2, W_MAX)
        y = y_all[a]
        d = (n[:, 0] * y[:, 0] + n[:, 1] * y[:, 1]) + n[:, 2] * y[:, 2]
        dst = label[a]
        s = 4
        for i in range(3):
            for k in range(i, 3):
                np.add.at(out[:, s], dst, _rint64(((w * n[:, i]) * n[:, k]) * S))
                s += 1
        for i in range(3):
            np.add.at(out[:, 10 + i], dst, _rint64(((w * d) * n[:, i]) * S))
        np.add.at(out[:, 13], dst, _rint64(w * S))
    return out


def leaders(vertices, label, origin, cell):
    """(V,) bool: label[v] == v and v inside the grid."""
    inside = SR.cells(vertices, origin, cell)[0]
    label = np.asarray(label, np.int64)
    return inside & (label == np.arange(len(label)))


def exported_sums(sums_, label):
    """What ngp_meshquadric_sums writes: the row where label[v] == v, zeros elsewhere."""
    label = np.asarray(label, np.int64)
    return np.where((label == np.arange(len(label)))[:, None], sums_, 0)


def place(vertices, label, origin, cell, sums_):
    """positions (V, 3) f32 (0 where not a leader: the library leaves those rows alone), state (V,) u8, totals (3,) int64."""
    x32 = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    n_v = len(x32)
    lead = np.nonzero(leaders(x32, label, origin, cell))[0]
    c = SR.cells(x32, origin, cell)[1][lead].astype(np.float64)
    o = np.asarray(origin, np.float32).reshape(3).astype(np.float64)
    h = np.float64(np.float32(cell))
    s = sums_[lead]
    sd = s.astype(np.float64)
    n = sd[:, 0]
    mean = (sd[:, 1:4] / n[:, None]) / np.float64(Q)
    m = mean - np.float64(0.5)
    r = EPS * sd[:, 13]
    M00, M01, M02 = sd[:, 4] + r, sd[:, 5], sd[:, 6]
    M11, M12, M22 = sd[:, 7] + r, sd[:, 8], sd[:, 9] + r
    g0, g1, g2 = sd[:, 10] + r * m[:, 0], sd[:, 11] + r * m[:, 1], sd[:, 12] + r * m[:, 2]
    with np.errstate(all="ignore"):
        d0 = M00
        l10 = M01 / d0
        l20 = M02 / d0
        d1 = M11 - l10 * M01
        t = M12 - l20 * M01
        l21 = t / d1
        d2 = (M22 - l20 * M02) - l21 * t
        z0 = g0
        z1 = g1 - l10 * z0
        z2 = (g2 - l20 * z0) - l21 * z1
        y2 = z2 / d2
        y1 = z1 / d1 - l21 * y2
        y0 = (z0 / d0 - l10 * y1) - l20 * y2
        y = np.stack([y0, y1, y2], 1)
        good = (d0 > 0) & (d1 > 0) & (d2 > 0) & (np.abs(y) <= 1).all(1)            # NaN and Inf compare false
    has_faces = s[:, 13] != 0
    st = np.where(has_faces, np.where(good, QUADRIC, MEAN_OUTSIDE), MEAN_NO_FACES).astype(np.uint8)
    with np.errstate(all="ignore"):
        in_cell = np.where((st == QUADRIC)[:, None], y + np.float64(0.5), mean)
        pos = (o[None, :] + (c + in_cell) * h).astype(np.float32)
    positions = np.zeros((n_v, 3), np.float32)
    state = np.zeros(n_v, np.uint8)
    positions[lead] = pos
    state[lead] = st
    totals = np.array([(st == k).sum() for k in (QUADRIC, MEAN_NO_FACES, MEAN_OUTSIDE)], np.int64)
    return positions, state, totals


def cluster_placement(vertices, faces, origin, cell, label=None):
    """-> positions (V, 3) f32, state (V,) u8, label (V,) i32, sums (V, 14) int64, totals (3,) int64."""
    if label is None:
        label = SR.vertex_labels(vertices, origin, cell)
    s = sums(vertices, faces, label, origin, cell)
    positions, state, totals = place(vertices, label, origin, cell, s)
    return positions, state, np.asarray(label, np.int32), s, totals


def simplify(vertices, faces, origin, cell, normals=None, colors=None, placement="quadric"):
    """tests/mesh_simplify_reference.simplify with the positions of `placement`; also returns the states of the output vertices."""
    v1, f1, n1, c1, label, clusters = SR.simplify(vertices, faces, origin, cell, normals, colors)
    positions, state, _, _, _ = cluster_placement(vertices, faces, origin, cell, label)
    # the output vertices: the labels a surviving face references, ascending
    f64 = np.asarray(faces, np.int64).reshape(-1, 3)
    n_v = len(label)
    ok = ((f64 >= 0) & (f64 < n_v)).all(1)
    lab = np.full(f64.shape, -1, np.int64)
    lab[ok] = label[f64[ok]]
    ok &= (lab >= 0).all(1) & (lab[:, 0] != lab[:, 1]) & (lab[:, 1] != lab[:, 2]) & (lab[:, 0] != lab[:, 2])
    used = np.unique(lab[ok])
    assert len(used) == len(v1)
    if placement == "quadric":
        v1 = positions[used]
    else:
        assert placement == "mean"
    return v1, f1, n1, c1, label, clusters, state[used]
