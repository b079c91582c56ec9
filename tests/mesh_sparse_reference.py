"""Numpy restatement of libngp_meshsparse.so (csrc/meshsparse/ngp_meshsparse.h), built on tests/mc_reference.py: the bricks of a
lattice, the dilation of a brick mask, the dense mesh restricted to a brick mask (faces by owning cell, the vertices they
reference in dense relative order, with the keys the library writes) and the mask from the occupancy bitfield in the header's f64
expressions.  Test infrastructure only."""
import numpy as np

from tests import mc_reference as R

BRICK = 8


def brick_dims(shape):
    """(nbz, nby, nbx) of a (nz, ny, nx) lattice."""
    return tuple((n + BRICK - 1) // BRICK for n in shape)


def dilate(mask):
    """26-neighbourhood dilation of a (nbz, nby, nbx) bool mask, clipped to the grid."""
    m = np.asarray(mask, bool)
    p = np.pad(m, 1)
    out = np.zeros_like(m)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= p[dz:dz + m.shape[0], dy:dy + m.shape[1], dx:dx + m.shape[2]]
    return out


def vertex_keys(vol, threshold):
    """3 * (owning point's linear index) + axis of the dense mesh's vertices, in its order (ascending)."""
    ins = np.ascontiguousarray(vol, np.float32) > np.float32(threshold)
    own = np.zeros(ins.shape + (3,), bool)
    own[:, :, :-1, 0] = ins[:, :, :-1] != ins[:, :, 1:]
    own[:, :-1, :, 1] = ins[:, :-1, :] != ins[:, 1:, :]
    own[:-1, :, :, 2] = ins[:-1, :, :] != ins[1:, :, :]
    return np.nonzero(own.reshape(-1))[0].astype(np.int64)


def face_cells(vol, threshold):
    """Per face of the dense mesh, in its order: the cell's (cz, cy, cx)."""
    nz, ny, nx = vol.shape
    cnt = R.TRI_COUNT[R.cube_indices(np.ascontiguousarray(vol, np.float32), np.float32(threshold))].reshape(-1)
    cells = np.repeat(np.arange(cnt.size), cnt)
    return cells // ((nx - 1) * (ny - 1)), (cells // (nx - 1)) % (ny - 1), cells % (nx - 1)


def restrict_indices(vol, threshold, mask):
    """The restriction as indices into the dense mesh: which faces are kept (bool per dense face), the dense indices of the vertices
    they reference (ascending), the kept faces renumbered (i32), the kept vertices' keys and per kept face the linear index of its
    cell's lowest corner.  `faces` of the dense mesh come from the restatement: they are integers, the same on every extractor."""
    vol = np.ascontiguousarray(vol, np.float32)
    nz, ny, nx = vol.shape
    mask = np.asarray(mask, bool)
    assert mask.shape == brick_dims(vol.shape)
    f = R.marching_cubes(vol, threshold, (0, 0, 0), (1, 1, 1))[1]
    keys = vertex_keys(vol, threshold)
    cz, cy, cx = face_cells(vol, threshold)
    keep = mask[cz // BRICK, cy // BRICK, cx // BRICK]
    fk = f[keep].astype(np.int64)
    used = np.unique(fk)
    remap = np.full(len(keys), -1, np.int64)
    remap[used] = np.arange(len(used))
    cell = ((cz * ny + cy) * nx + cx)[keep].astype(np.int64)
    return keep, used, remap[fk].astype(np.int32).reshape(-1, 3), keys[used], cell


def restrict(vol, threshold, lo, hi, mask):
    """The dense mesh restricted to the bricks of `mask`: vertices, faces (i32, renumbered), normals, vertex keys, and per face the
    linear index of its cell's lowest corner.  The faces whose cell lies in a meshed brick, in dense order, and the vertices they
    reference, in dense order."""
    v, _, n, _ = R.marching_cubes(vol, threshold, lo, hi)
    _, used, faces, keys, cell = restrict_indices(vol, threshold, mask)
    return v[used], faces, n[used], keys, cell


def morton(cx, cy, cz):
    def expand(v):
        v = np.asarray(v, np.uint64)
        out = np.zeros_like(v)
        for b in range(10):
            out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
        return out
    return expand(cx) | (expand(cy) << np.uint64(1)) | (expand(cz) << np.uint64(2))


def occupancy_grids(bitfield, cascades, G):
    """(cascades, G, G, G) bool indexed [k, cz, cy, cx]: bit k * G^3 + morton(cx, cy, cz), byte >> 3, bit & 7."""
    bits = np.unpackbits(np.asarray(bitfield, np.uint8), bitorder="little")[:cascades * G ** 3].reshape(cascades, G ** 3)
    cz, cy, cx = np.meshgrid(np.arange(G), np.arange(G), np.arange(G), indexing="ij")
    return bits[:, morton(cx, cy, cz).astype(np.int64)].astype(bool)


def grown_extents(shape, lo, hi, margin_voxels):
    """Per axis (x, y, z): (g0, g1) f64 arrays over the bricks of the axis, by the header's expressions."""
    nz, ny, nx = shape
    out = []
    for a, n in enumerate((nx, ny, nz)):
        l, u = np.float64(np.float32(lo[a])), np.float64(np.float32(hi[a]))
        h = (u - l) / np.float64(n - 1)
        b = np.arange((n + BRICK - 1) // BRICK)
        e0 = l + (BRICK * b).astype(np.float64) * h
        e1 = l + np.minimum(BRICK * b + BRICK, n - 1).astype(np.float64) * h
        m = np.float64(margin_voxels) * h
        out.append((e0 - m, e1 + m))
    return out


def occupancy_mask(bitfield, cascades, G, scale, shape, lo, hi, margin_voxels=1, grids=None):
    """(nbz, nby, nbx) bool: the header's rule.  grids: occupancy_grids(bitfield, cascades, G) when the caller has them already."""
    grids = occupancy_grids(bitfield, cascades, G) if grids is None else grids
    (x0, x1), (y0, y1), (z0, z1) = grown_extents(shape, lo, hi, margin_voxels)
    scale = np.float64(np.float32(scale))
    s_of = [min(np.float64(2.0) ** (k - 1), scale) for k in range(cascades)]
    Gd = np.float64(G)

    def cell(u, s):
        return int(min(max(np.floor((u / s + 1.0) * 0.5 * Gd), 0.0), Gd - 1.0))

    mask = np.zeros((len(z0), len(y0), len(x0)), bool)
    for bz in range(len(z0)):
        for by in range(len(y0)):
            for bx in range(len(x0)):
                g0 = (x0[bx], y0[by], z0[bz])
                g1 = (x1[bx], y1[by], z1[bz])
                k = cascades - 1
                for c in range(cascades):
                    if all(-s_of[c] <= g0[a] and g1[a] <= s_of[c] for a in range(3)):
                        k = c
                        break
                s = s_of[k]
                c0 = [cell(g0[a], s) for a in range(3)]
                c1 = [cell(g1[a], s) for a in range(3)]
                mask[bz, by, bx] = grids[k, c0[2]:c1[2] + 1, c0[1]:c1[1] + 1, c0[0]:c1[0] + 1].any()
    return mask


def set_bits(cascades, G, cells):
    """A bitfield (cascades * G^3 / 8 uint8) with the cells (k, cx, cy, cz) set."""
    out = np.zeros(cascades * G ** 3 // 8, np.uint8)
    for k, cx, cy, cz in cells:
        i = k * G ** 3 + int(morton(cx, cy, cz))
        out[i >> 3] |= 1 << (i & 7)
    return out
