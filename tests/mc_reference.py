"""Vectorised numpy restatement of the marching cubes of libngp_mesh.so: the same generated table (ngp_pl_amd.mc_tables), the
same numbering (vertices by owning lattice point then axis x<y<z; triangles by cell then table order), the same f32 formulas
for the edge parameter, the vertex and the normal.  Test infrastructure only."""
import numpy as np

from ngp_pl_amd import mc_tables

_EDGE_MASK, _TRIS, _MAXT = mc_tables.tables()
TRI_COUNT = np.array([len(t) for t in _TRIS], np.int64)
TRIS = np.full((256, 3 * _MAXT), -1, np.int64)
for _c, _t in enumerate(_TRIS):
    if _t:
        TRIS[_c, :3 * len(_t)] = np.array(_t, np.int64).reshape(-1)
EDGE_OWNER = np.array([mc_tables.corner_xyz(a) for a, _ in mc_tables.EDGES], np.int64)     # (12, 3) corner offset (x, y, z)
EDGE_AXIS = np.arange(12) // 4


def spacing(shape, lo, hi):
    """Per-axis lattice spacing (x, y, z) in f32: (hi - lo) / (n - 1)."""
    nz, ny, nx = shape
    n = np.array([nx, ny, nz], np.float32)
    return (np.asarray(hi, np.float32) - np.asarray(lo, np.float32)) / (n - np.float32(1))


def cube_indices(vol, threshold):
    ins = (vol > np.float32(threshold)).astype(np.int64)
    cube = np.zeros([s - 1 for s in vol.shape], np.int64)
    for c in range(8):
        x, y, z = mc_tables.corner_xyz(c)
        cube |= ins[z:z + vol.shape[0] - 1, y:y + vol.shape[1] - 1, x:x + vol.shape[2] - 1] << c
    return cube


def _gradient(vol, h):
    g = np.zeros(vol.shape + (3,), np.float32)
    for ax, npax in enumerate((2, 1, 0)):
        v = np.moveaxis(vol, npax, -1)
        out = np.zeros_like(v)
        out[..., 1:-1] = (v[..., 2:] - v[..., :-2]) / (np.float32(2) * h[ax])
        out[..., 0] = (v[..., 1] - v[..., 0]) / h[ax]
        out[..., -1] = (v[..., -1] - v[..., -2]) / h[ax]
        g[..., ax] = np.moveaxis(out, -1, npax)
    return g


def marching_cubes(vol, threshold, lo, hi):
    """vol (nz, ny, nx) f32 -> vertices (V,3) f32, faces (F,3) i32, normals (V,3) f32, cube index per cell."""
    vol = np.ascontiguousarray(vol, np.float32)
    thr = np.float32(threshold)
    nz, ny, nx = vol.shape
    lo = np.asarray(lo, np.float32)
    h = spacing(vol.shape, lo, hi)
    ins = vol > thr
    own = np.zeros(vol.shape + (3,), bool)
    own[:, :, :-1, 0] = ins[:, :, :-1] != ins[:, :, 1:]
    own[:, :-1, :, 1] = ins[:, :-1, :] != ins[:, 1:, :]
    own[:-1, :, :, 2] = ins[:-1, :, :] != ins[1:, :, :]
    flat = own.reshape(-1)
    vid = np.cumsum(flat) - 1
    sel = np.nonzero(flat)[0]
    p, axis = sel // 3, sel % 3
    k, j, i = p // (nx * ny), (p // nx) % ny, p % nx
    stride = np.array([1, nx, nx * ny])[axis]
    sa, sb = vol.reshape(-1)[p], vol.reshape(-1)[p + stride]
    t = np.clip((thr - sa) / (sb - sa), np.float32(0), np.float32(1)).astype(np.float32)
    idx = np.stack([i, j, k], 1)
    pa = lo + idx.astype(np.float32) * h
    idxb = idx.copy()
    idxb[np.arange(len(idx)), axis] += 1
    pb = lo + idxb.astype(np.float32) * h
    verts = (pa + t[:, None] * (pb - pa)).astype(np.float32)
    g = _gradient(vol, h).reshape(-1, 3)
    ga, gb = g[p], g[p + stride]
    gv = ga + t[:, None] * (gb - ga)
    nrm = np.sqrt(gv[:, 0] * gv[:, 0] + gv[:, 1] * gv[:, 1] + gv[:, 2] * gv[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        normals = np.where(nrm[:, None] > 0, -gv / nrm[:, None], np.float32(0)).astype(np.float32)
    cube = cube_indices(vol, thr)
    cnt = TRI_COUNT[cube].reshape(-1)
    cells = np.repeat(np.arange(cnt.size), cnt)
    first = np.cumsum(cnt) - cnt
    r = np.arange(cells.size) - first[cells]
    cz, cy, cx = cells // ((nx - 1) * (ny - 1)), (cells // (nx - 1)) % (ny - 1), cells % (nx - 1)
    cubes = cube.reshape(-1)[cells]
    faces = np.zeros((cells.size, 3), np.int64)
    for c in range(3):
        e = TRIS[cubes, 3 * r + c]
        off = EDGE_OWNER[e]
        q = ((cz + off[:, 2]) * ny + (cy + off[:, 1])) * nx + (cx + off[:, 0])
        faces[:, c] = vid[q * 3 + EDGE_AXIS[e]]
    return verts, faces.astype(np.int32), normals, cube


def edge_use(faces):
    """{(a, b): count} of directed triangle edges."""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    key = e[:, 0] * (1 << 32) + e[:, 1]
    u, c = np.unique(key, return_counts=True)
    return dict(zip(zip((u >> 32).tolist(), (u & 0xffffffff).tolist()), c.tolist()))


def is_closed_oriented(faces):
    """Every undirected edge used by exactly two faces, once in each direction."""
    use = edge_use(faces)
    return all(c == 1 and use.get((b, a)) == 1 for (a, b), c in use.items())


def euler(verts, faces):
    use = edge_use(faces)
    n_edges = len({(min(a, b), max(a, b)) for a, b in use})
    return len(verts) - n_edges + len(faces)


def signed_volume(verts, faces):
    v = verts.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def area(verts, faces):
    v = verts.astype(np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum())
