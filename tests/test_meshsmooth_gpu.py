"""GPU: libngp_meshsmooth.so bit for bit against the numpy restatement (tests/mesh_smooth_reference.py): degrees, flags, the four
totals, smoothed positions and geometric normals as int32 words or exactly, on the smallest inputs at which each mechanism can fail
(block and wave edges, rows on both sides of the length from which a wave sums a row, a hub of 5000 neighbours, bad faces and
vertices, rounding ties and the clamp, every option), on marching-cubes meshes twice, on a side stream and with the faces permuted,
and through extract_mesh(smooth=...) and the CLI.  Every sum is an integer sum and every other value a single expression: nothing
here has a tolerance."""
import re

import numpy as np
import pytest
import torch

from tests import mc_reference as R
from tests import mesh_smooth_reference as SR

pytestmark = pytest.mark.gpu


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def to_mesh(v, f, n=None, c=None, device="cuda"):
    from ngp_pl_amd import mesh
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return mesh.Mesh(t(v), t(f), t(n), t(c))


def same_words(a, b):
    return (a is None) == (b is None) and (a is None or (a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))))


def same_mesh(a, b):
    return torch.equal(a.faces, b.faces) and same_words(a.vertices, b.vertices) and same_words(a.normals, b.normals) and same_words(a.colors, b.colors)


def check(v, f, cell, origin, pairs=2, lam=0.5, mu=-0.53, pin=True, trace=None):
    """mesh_topology, smooth_taubin and vertex_normals (of the input and of the result) against the restatement, exactly; returns
    the restatement's degree, flags, totals and positions."""
    from ngp_pl_amd import mesh
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    origin = np.asarray(origin, np.float32)
    cell = np.float32(cell)
    degree, flags, totals, _ = SR.topology(v, f, origin, cell, pin)
    want = SR.taubin(v, f, origin, cell, pairs, lam, mu, pin, trace)
    m = to_mesh(v, f, SR.normals(v, f))
    t = mesh.mesh_topology(m, float(cell), origin=origin.tolist(), pin_boundary=pin)
    assert t.degree.dtype == torch.int32 and t.flags.dtype == torch.uint8
    assert np.array_equal(t.degree.cpu().numpy(), degree), "%d degrees differ" % (t.degree.cpu().numpy() != degree).sum()
    assert np.array_equal(t.flags.cpu().numpy(), flags), "%d flags differ" % (t.flags.cpu().numpy() != flags).sum()
    assert [t.n_edges, t.n_boundary_edges, t.n_free, t.n_boundary_vertices] == totals.tolist()
    got = mesh.smooth_taubin(m, float(cell), pairs, lam, mu, origin=torch.from_numpy(origin), pin_boundary=pin)
    assert got.vertices.dtype == torch.float32 and got.vertices.shape == want.shape
    assert np.array_equal(bits(got.vertices), bits(want)), "%d position words differ" % (bits(got.vertices) != bits(want)).sum()
    assert got.faces.dtype == torch.int32 and np.array_equal(got.faces.cpu().numpy(), f) and got.colors is None
    assert np.array_equal(bits(mesh.vertex_normals(m)), bits(m.normals))
    want_n = SR.normals(want, f)
    assert np.array_equal(bits(got.normals), bits(want_n)), "%d normal words differ" % (bits(got.normals) != bits(want_n)).sum()
    return degree, flags, totals, want


def sheet(n_v, n_f, seed, w=37):
    """n_v jittered points of a w-wide sheet of unit spacing and n_f faces (j, j + 1, j + w) over them, indices modulo n_v."""
    g = np.random.RandomState(seed)
    i = np.arange(n_v)
    v = np.stack([i % w, i // w, np.zeros(n_v)], 1) + g.uniform(-0.4, 0.4, (n_v, 3))
    j = np.arange(n_f)
    f = np.stack([j % n_v, (j + 1) % n_v, (j + w) % n_v], 1)
    return v.astype(np.float32), f.astype(np.int32), g


def grid_sheet(nx, ny, seed, jitter=0.3):
    """A triangulated nx x ny sheet of unit spacing, jittered: interior vertices of degree 6, an open boundary."""
    g = np.random.RandomState(seed)
    y, x = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    v = np.stack([x.ravel(), y.ravel(), np.zeros(nx * ny)], 1) + g.uniform(-jitter, jitter, (nx * ny, 3))
    i = (y[:-1, :-1] * nx + x[:-1, :-1]).ravel()
    f = np.concatenate([np.stack([i, i + 1, i + nx], 1), np.stack([i + 1, i + nx + 1, i + nx], 1)])
    return v.astype(np.float32), f.astype(np.int32), g


@pytest.mark.parametrize("n", [63, 64, 65, 2047, 2048, 2049, 4097])
def test_block_and_wave_edges(n):
    v, f, _ = sheet(n, n, n)
    degree, flags, totals, _ = check(v, f, 1.0, (-1, -1, -1), pin=False)
    assert totals[2] == n and degree.min() >= 2
    # faces and vertices on different sides of a block edge
    v2, f2, _ = sheet(n, 2 * n - 1, n + 1)
    check(v2, f2, 0.7, (-1, -1, -1), pin=True)
    v3, f3, _ = sheet(2 * n - 1, n, n + 2)
    check(v3, f3, 1.3, (-1, -1, -1), pin=False)


def test_row_scan_takes_a_second_block_per_thread():
    """699 051 disjoint triangles are 2 097 153 vertices, 1025 blocks of 2048: the one-workgroup scan of the blocks' degree sums
    takes two blocks per thread.  The row offsets are not an output; a wrong one sends a vertex to another triangle's neighbours,
    and the pass then moves it elsewhere.  Topology and one pair of passes only: the restatement is slow at this size."""
    from ngp_pl_amd import mesh
    n_v = 3 * 699051
    assert -(-n_v // 2048) == 1025
    v = np.random.RandomState(7).uniform(-1, 1, (n_v, 3)).astype(np.float32)
    f = np.arange(n_v, dtype=np.int32).reshape(-1, 3)
    origin, cell = np.float32([-1.5, -1.5, -1.5]), np.float32(0.01)
    degree, flags, totals, _ = SR.topology(v, f, origin, cell, False)
    assert totals.tolist() == [n_v] * 4 and (degree == 2).all()
    m = to_mesh(v, f)
    t = mesh.mesh_topology(m, float(cell), origin=origin.tolist(), pin_boundary=False)
    assert np.array_equal(t.degree.cpu().numpy(), degree) and np.array_equal(t.flags.cpu().numpy(), flags)
    assert [t.n_edges, t.n_boundary_edges, t.n_free, t.n_boundary_vertices] == totals.tolist()
    got = mesh.smooth_taubin(m, float(cell), 1, 0.5, -0.53, origin=torch.from_numpy(origin), pin_boundary=False)
    want = SR.taubin(v, f, origin, cell, 1, 0.5, -0.53, False)
    assert np.array_equal(bits(got.vertices), bits(want)), "%d position words differ" % (bits(got.vertices) != bits(want)).sum()


def fan(n, g, centre):
    """A closed fan of n triangles round a hub with a second ring outside it: the hub has n neighbours, the inner ring's vertices
    5, the outer ring's 4 (and are the boundary).  The hub is the LAST vertex."""
    a = 2 * np.pi * np.arange(n) / n
    ring = lambda r, shift: np.stack([r * np.cos(a + shift), r * np.sin(a + shift), np.zeros(n)], 1)
    v = np.concatenate([ring(10, 0), ring(11, np.pi / n), [[0, 0, 3]]]) + g.uniform(-0.02, 0.02, (2 * n + 1, 3)) + np.asarray(centre, np.float64)
    i = np.arange(n)
    nxt = (i + 1) % n
    f = np.concatenate([np.stack([np.full(n, 2 * n), i, nxt], 1), np.stack([i, n + i, nxt], 1), np.stack([n + i, n + nxt, nxt], 1)])
    return v.astype(np.float32), f.astype(np.int32)


def test_long_rows():
    g = np.random.RandomState(11)
    parts, offset = [], 0
    # 31, 32 and 33 neighbours: either side of the length from which a wave sums the row; 64 and 65: one round of the wave and two
    for k, n in enumerate((5000, 31, 32, 33, 64, 65, 129)):
        v, f = fan(n, g, (30 * k, 0, 0))
        parts.append((v, f + offset))
        offset += len(v)
    v, f = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    f = f[g.permutation(len(f))]
    for pin in (True, False):
        degree, flags, totals, want = check(v, f, 0.25, (-20, -20, -20), pairs=3, pin=pin)
        assert sorted(set(degree.tolist())) == [4, 5, 31, 32, 33, 64, 65, 129, 5000] and degree[10000] == 5000
        assert ((flags & 4) != 0).sum() == (len(v) if not pin else len(v) - (degree == 4).sum())
        assert np.abs(want[10000] - v[10000]).max() > 0.1                    # the hub moved towards its ring's plane


@pytest.fixture(scope="module")
def mc_meshes():
    out = {}
    for name, n in (("sphere", 24), ("torus", 32)):
        z, y, x = np.meshgrid(*[np.linspace(-1, 1, n, dtype=np.float32)] * 3, indexing="ij")
        if name == "sphere":
            vol = np.float32(0.8) - np.sqrt(x * x + y * y + z * z)
        else:
            vol = np.float32(0.25) - np.sqrt((np.sqrt(x * x + y * y) - np.float32(0.6)) ** 2 + z * z)
        v, f, nrm, _ = R.marching_cubes(vol.astype(np.float32), 0.0, (-1, -1, -1), (1, 1, 1))
        h = 2.0 / (n - 1)
        noisy = (v + np.random.RandomState(n).uniform(-0.3, 0.3, v.shape) * h).astype(np.float32)
        out[name] = (noisy, f, nrm, h)
    return out


def test_bad_faces(mc_meshes):
    v, f, _, h = mc_meshes["sphere"]
    v, f = v.copy(), f.copy()
    g = np.random.RandomState(12)
    n_v = len(v)
    fr = g.permutation(len(f))[:360]
    for k, bad in enumerate((-1, n_v + 50, 2 ** 31 - 1, -2 ** 31, n_v + 57)):    # out of range (50 vertices follow) and negative
        f[fr[40 * k:40 * k + 40], g.randint(0, 3, 40)] = bad
    f[fr[200:240], 1] = f[fr[200:240], 0]                                        # a repeated index
    f[fr[240:280], 2] = f[fr[240:280], 1]
    twice = f[fr[280:320]]                                                       # the same face again, as it is and rotated
    third = np.stack([f[fr[320:360], 0], f[fr[320:360], 1], g.randint(0, n_v, 40)], 1).astype(np.int32)      # a third face on an edge
    f = np.concatenate([f, twice, twice[:, [1, 2, 0]], third])
    v = np.concatenate([v, g.uniform(-1, 1, (50, 3)).astype(np.float32)])        # isolated vertices
    degree, flags, totals, want = check(v, f, h, (-1, -1, -1), pin=True)
    assert (degree[n_v:] == 0).all() and (flags[n_v:] == 1).all() and np.array_equal(bits(want[n_v:]), bits(v[n_v:]))
    assert 0 < totals[1] < totals[0] and 0 < totals[2] < n_v
    # known answers: a face given twice has no boundary edge; three faces on one edge leave that edge off the boundary
    quad = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 1]])
    for faces, edges, boundary_edges, free in (([[0, 1, 2], [1, 2, 0]], 3, 0, 3), ([[0, 1, 2], [1, 3, 2], [2, 1, 4]], 7, 6, 0),
                                               ([[0, 1, 2], [1, 3, 2], [2, 1, 4], [0, 1, 2], [2, 1, 3], [1, 4, 2]], 7, 0, 5)):
        _, _, totals, _ = check(quad, np.int32(faces), 1.0, (0, 0, 0), pin=True)
        assert totals[:3].tolist() == [edges, boundary_edges, free]
    # no faces at all: nothing is free, every word stays
    degree, flags, totals, want = check(v, np.zeros((0, 3), np.int32), h, (-1, -1, -1))
    assert (degree == 0).all() and totals.tolist() == [0, 0, 0, 0] and np.array_equal(bits(want), bits(v))


def test_bad_vertices(mc_meshes):
    from ngp_pl_amd import mesh
    v, f, _, h = mc_meshes["sphere"]
    v = v.copy()
    g = np.random.RandomState(13)
    nan, inf = np.float32("nan"), np.float32("inf")
    rows = g.permutation(len(v))[:240]
    # 2^14 cells of h are 1394 units: 1500 is beyond the grid, 1300 inside it
    for k, bad in enumerate((nan, inf, -inf, np.float32(1500), np.float32(-1500), np.float32(3e38))):
        v[rows[40 * k:40 * k + 40], g.randint(0, 3, 40)] = bad
    v.view(np.int32)[rows[0], 0] = 0x7FC12345                                    # a NaN with a payload: copied word for word
    v[rows[-1]] = [1300, 0, 0]
    degree, flags, totals, want = check(v, f, h, (-1, -1, -1), pin=False)
    out = rows[:240]
    outside = (flags & 1) == 0
    assert outside.sum() == 239 and outside[out[:-1]].all() and not outside[rows[-1]]
    assert (degree[outside] == 0).all() and np.array_equal(bits(want[outside]), bits(v[outside]))
    # the faces of an outside vertex still give their other side, wherever the third corner is: on this closed surface every edge
    # between two inside vertices still occurs twice, and the neighbours of an outside vertex lose that one edge only
    assert totals[1] == 0 and totals[3] == 0 and totals[2] == len(v) - 239
    nb = np.unique(f[np.isin(f, out[:-1]).any(1)])
    nb = nb[~outside[nb]]
    clean_degree = SR.topology(mc_meshes["sphere"][0], f, np.float32([-1, -1, -1]), np.float32(h), False)[0]
    assert len(nb) > 239 and (degree[nb] >= 2).all() and (degree[nb] < clean_degree[nb]).any() and (degree <= clean_degree).all()
    # a NaN origin: every vertex is outside the grid and keeps its words; a cell so small that every vertex is beyond the grid
    _, flags, totals, _ = check(v, f, h, (nan, -1, -1))
    assert (flags == 0).all() and totals.tolist() == [0, 0, 0, 0]
    _, flags, totals, _ = check(v, f, 1e-6, (-1, -1, -1))
    assert (flags == 0).sum() >= len(v) - 10 and totals[0] <= 10
    # origin=None is the vertices' minimum, taken on the device
    clean = mc_meshes["sphere"][0]
    got = mesh.smooth_taubin(to_mesh(clean, f), float(np.float32(h)), 2)
    assert np.array_equal(bits(got.vertices), bits(SR.taubin(clean, f, clean.min(0), np.float32(h), 2, 0.5, -0.53)))
    t = mesh.mesh_topology(to_mesh(clean, f), float(np.float32(h)))
    assert np.array_equal(t.degree.cpu().numpy(), SR.topology(clean, f, clean.min(0), np.float32(h))[0])


def test_rounding_ties():
    g = np.random.RandomState(14)
    n = 600                                                                      # triples; the third corner of every other one is outside
    k = 2 * g.randint(-40000, 40000, (3 * n, 3)) + 1                             # odd multiples of cell / 65536: exact in float32
    v = (k / 65536.0).astype(np.float32)
    assert np.array_equal(v.astype(np.float64) * 65536, k)
    v[5::6] = np.float32("nan")
    f = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    trace = {}
    degree, flags, totals, _ = check(v, f, 1.0, (0, 0, 0), pairs=1, lam=0.5, mu=0.5, pin=False, trace=trace)
    assert sorted(set(degree.tolist())) == [0, 1, 2] and (degree == 1).sum() == n and (degree == 2).sum() == 3 * n // 2
    assert trace["ties"] > 0                    # degree 2: half the sum of two odd numbers minus an odd number is odd half the time, times 0.5
    # even and odd multiples mixed: a vertex of degree 1 meets a half whenever its neighbour is an odd number of quanta away
    k = g.randint(-40000, 40000, (3 * n, 3))
    v2 = (k / 65536.0).astype(np.float32)
    v2[5::6] = np.float32("nan")
    ones = np.repeat(np.arange(n) % 2 == 1, 3) & (np.arange(3 * n) % 3 != 2)
    odd = ((k[3::6] - k[4::6]) % 2 != 0).sum()
    trace2 = {}
    check(v2, f, 1.0, (0, 0, 0), pairs=1, lam=0.5, mu=0.0, pin=False, trace=trace2)
    assert ones.sum() == n and odd > 0 and trace2["ties"] >= 2 * odd
    check(v2, f, 1.0, (0, 0, 0), pairs=3, lam=0.5, mu=-0.5, pin=False)
    # a cell that is no power of two and an origin that is not 0
    check((v * np.float32(3) + np.float32(1.5)).astype(np.float32), f, 3.0, (1.5, 1.5, 1.5), pairs=1, lam=0.5, mu=0.5, pin=False)


def test_the_clamp():
    trace = {}
    v = np.float32([[16000, 0, 0], [-16000, 0, 0], [0, 1, 0], [16384, 5, 5], [16384, 6, 5], [16383.5, 5, 6], [-16384, -16384, -16384], [-16383, -16384, -16380],
                    [-16384, -16380, -16384]])
    f = np.int32([[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    degree, flags, totals, want = check(v, f, 1.0, (0, 0, 0), pairs=2, lam=-1.0, mu=-1.0, pin=False, trace=trace)
    assert trace["clamped"] > 0 and trace["at_qmax"] > 0 and totals[2] == 9
    assert want[0, 0] == 16384 and want[1, 0] == -16384 and want[6].tolist() == [-16384] * 3
    # a noisy patch next to the grid's upper corner, anti-smoothed: it grows into the corner
    trace = {}
    pv, pf, _ = grid_sheet(9, 7, 15)
    check(pv + np.float32([16375, 16377, 16383]), pf, 1.0, (0, 0, 0), pairs=4, lam=-1.0, mu=-1.0, pin=False, trace=trace)
    assert trace["clamped"] > 0
    trace = {}
    check(-pv - np.float32([16375, 16377, 16383]), pf, 1.0, (0, 0, 0), pairs=4, lam=-1.0, mu=-1.0, pin=False, trace=trace)
    assert trace["at_qmax"] > 0


@pytest.mark.parametrize("pin", [True, False])
@pytest.mark.parametrize("pairs", [1, 2, 7])
def test_options_on_an_open_mesh(pin, pairs):
    v, f, _ = grid_sheet(41, 53, 16)
    degree, flags, totals, want = check(v, f, 0.5, (-1, -1, -1), pairs=pairs, pin=pin)
    boundary = (flags & 2) != 0
    assert boundary.sum() == 2 * (41 + 53) - 4 == totals[1] and totals[2] == (len(v) - boundary.sum() if pin else len(v))
    moved = (bits(want) != bits(v)).any(1)
    assert moved[~boundary].all() and (moved[boundary].all() if not pin else not moved[boundary].any())


def test_zero_factors_and_zero_iterations():
    from ngp_pl_amd import mesh
    v, f, g = grid_sheet(23, 19, 17)
    _, flags, _, a = check(v, f, 0.5, (-1, -1, -1), pairs=2, lam=0.0, mu=0.0, pin=True)
    free = (flags & 4) != 0
    # free vertices still take the output formula: one trip through the grid
    assert (bits(a) != bits(v))[free].any() and np.array_equal(bits(a[~free]), bits(v[~free]))
    # half a quantum of 0.5 / 65536, and half a float32 ulp of a coordinate below 64 going in and coming out
    assert np.abs(a.astype(np.float64) - v).max() <= 0.25 / 65536 + 2 * 2.0 ** -19
    check(v, f, 0.5, (-1, -1, -1), pairs=2, lam=0.0, mu=-0.53)
    check(v, f, 0.5, (-1, -1, -1), pairs=2, lam=0.5, mu=0.0)
    check(v, f, 0.5, (-1, -1, -1), pairs=1, lam=1.0, mu=-1.0)
    n = g.normal(size=v.shape).astype(np.float32)
    c = g.uniform(0, 1, v.shape).astype(np.float32)
    m = to_mesh(v, f, n, c)
    same = mesh.smooth_taubin(m, 0.5, iterations=0)
    assert same_mesh(same, m) and same.vertices.data_ptr() != m.vertices.data_ptr()
    # empty meshes: nothing is launched
    z3, zi = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    for e in (to_mesh(z3, zi), to_mesh(z3, zi, z3, z3), to_mesh(z3, f)):
        out = mesh.smooth_taubin(e, 0.5)
        assert out.vertices.shape == (0, 3) and torch.equal(out.faces, e.faces) and (out.normals is None) == (e.normals is None)
        assert mesh.vertex_normals(e).shape == (0, 3) and mesh.mesh_topology(e, 0.5).degree.shape == (0,)
        assert mesh.mesh_topology(e, 0.5).n_edges == 0


def test_normals():
    from ngp_pl_amd import mesh
    nan, inf = np.float32("nan"), np.float32("inf")
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [nan, 0, 0], [5, 5, 5], [3e38, 0, 0], [0, 3e38, 0], [7, 7, 7], [8, 7, 7], [7, 8, 7],
                    [0, 0, inf], [1e-30, 0, 0], [0, 1e-30, 0]])
    f = np.int32([[8, 9, 10], [8, 10, 9], [0, 1, 3], [0, 1, 1], [0, 1, 4], [0, 1, 14], [-1, 1, 2], [1, 3, 2], [0, 6, 7], [0, 1, 11], [0, 12, 13],
                  [2 ** 31 - 1, 0, 1], [5, 5, 5]])
    want = SR.normals(v, f)
    assert want[8:11].tolist() == [[0, 0, 0]] * 3 and want[5].tolist() == [0, 0, 0] and want[1].tolist() == [0, 0, 1]
    got = mesh.vertex_normals(to_mesh(v, f))
    assert got.dtype == torch.float32 and np.array_equal(bits(got), bits(want))
    # on a curved mesh, block edges included; absent normals stay absent; recompute_normals=False copies the input's words
    sv, sf, g = sheet(4097, 6001, 18)
    sv[:, 2] = np.sin(sv[:, 0]) + np.cos(sv[:, 1])
    n_in = g.normal(size=sv.shape).astype(np.float32)
    c_in = g.uniform(0, 1, sv.shape).astype(np.float32)
    assert np.array_equal(bits(mesh.vertex_normals(to_mesh(sv, sf))), bits(SR.normals(sv, sf)))
    bare = mesh.smooth_taubin(to_mesh(sv, sf), 1.0, 2, origin=(-2, -2, -2))
    assert bare.normals is None and bare.colors is None
    want_v = SR.taubin(sv, sf, np.float32([-2, -2, -2]), 1.0, 2, 0.5, -0.53)
    assert np.array_equal(bits(bare.vertices), bits(want_v))
    m = to_mesh(sv, sf, n_in, c_in)
    kept = mesh.smooth_taubin(m, 1.0, 2, origin=(-2, -2, -2), recompute_normals=False)
    assert same_words(kept.vertices, bare.vertices) and same_words(kept.normals, m.normals) and same_words(kept.colors, m.colors)
    assert kept.normals.data_ptr() != m.normals.data_ptr()
    new = mesh.smooth_taubin(m, 1.0, 2, origin=(-2, -2, -2))
    assert np.array_equal(bits(new.normals), bits(SR.normals(want_v, sf))) and same_words(new.colors, m.colors)


@pytest.mark.parametrize("scene", ["sphere", "torus"])
def test_marching_cubes_meshes_twice_on_a_side_stream_and_permuted(scene, mc_meshes):
    from ngp_pl_amd import mesh
    v, f, nrm, h = mc_meshes[scene]
    degree, flags, totals, want = check(v, f, h, (-1, -1, -1), pairs=10, pin=True)
    assert totals[1] == 0 and totals[2] == len(v) and totals[0] * 2 == len(f) * 3          # closed and manifold
    check(v, f, h, (-1, -1, -1), pairs=10, pin=True)
    m = to_mesh(v, f, nrm)
    cell = float(np.float32(h))
    a = mesh.smooth_taubin(m, cell, 10, origin=(-1, -1, -1))
    ta = mesh.mesh_topology(m, cell, origin=(-1, -1, -1))
    assert np.array_equal(bits(a.vertices), bits(want))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = mesh.smooth_taubin(m, cell, 10, origin=(-1, -1, -1))
        tb = mesh.mesh_topology(m, cell, origin=(-1, -1, -1))
        nb = mesh.vertex_normals(mesh.Mesh(b.vertices, b.faces))
    side.synchronize()
    assert same_mesh(a, b) and torch.equal(ta.degree, tb.degree) and torch.equal(ta.flags, tb.flags) and same_words(nb, a.normals)
    g = np.random.RandomState(19)
    shuffled = f[g.permutation(len(f))]
    shuffled = np.where((g.randint(0, 2, len(f)) == 1)[:, None], shuffled[:, [1, 2, 0]], shuffled)
    p = mesh.smooth_taubin(to_mesh(v, shuffled, nrm), cell, 10, origin=(-1, -1, -1))
    tp = mesh.mesh_topology(to_mesh(v, shuffled), cell, origin=(-1, -1, -1))
    assert same_words(p.vertices, a.vertices) and same_words(p.normals, a.normals) and torch.equal(tp.degree, ta.degree)
    assert torch.equal(tp.flags, ta.flags) and (tp.n_edges, tp.n_free) == (ta.n_edges, ta.n_free)


def make_model(seed=3):
    from ngp_pl_amd.networks import NGP
    torch.manual_seed(seed)
    m = NGP(scale=0.5).cuda()
    m.register_training_buffers()
    return m


@pytest.fixture
def true_density(monkeypatch):
    """The model's density lattice replaced by the procedural scene's true density, as tests/test_mesh_gpu.py samples it."""
    from ngp_pl_amd import mesh, synthetic as syn

    def volume(model, resolution=512, bounds=None, chunk=0):
        nx, ny, nz = mesh._resolution(resolution)
        xyz = mesh.lattice_points((nx, ny, nz), mesh._bounds(model, bounds))
        return syn.density(xyz).view(nz, ny, nx).contiguous()

    monkeypatch.setattr(mesh, "density_volume", volume)


def test_extract_mesh_chain(true_density):
    from ngp_pl_amd import mesh
    model = make_model()
    res = 48
    plain = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, colors=True)
    none = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, colors=True, smooth=None)
    assert same_mesh(plain, none)                                              # without the option: today's output
    lo, hi = mesh._box(model)
    cell = max((b - a) / (res - 1) for a, b in zip(lo, hi))
    for smooth, kw in ((4, dict(iterations=4)), (dict(iterations=3, lam=0.6, mu=-0.63, pin_boundary=False), None)):
        kw = kw or dict(iterations=3, lam=0.6, mu=-0.63, pin_boundary=False)
        got = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, colors=True, smooth=smooth)
        want = mesh.smooth_taubin(plain, cell, origin=lo, **kw)
        assert same_mesh(got, want) and not same_words(got.vertices, plain.vertices)
        # smoothing is last; the colours are those of the surface the field defines, carried through
        assert same_words(got.colors, plain.colors) and torch.equal(got.faces, plain.faces)
        assert same_words(got.colors, mesh.vertex_colors(model, plain.vertices, plain.normals))
        assert same_words(got.normals, mesh.vertex_normals(got)) and not same_words(got.normals, plain.normals)
        assert np.array_equal(bits(got.vertices), bits(SR.taubin(plain.vertices.cpu().numpy(), plain.faces.cpu().numpy(), np.float32(lo),
                                                                  np.float32(cell), kw["iterations"], kw.get("lam", 0.5), kw.get("mu", -0.53),
                                                                  kw.get("pin_boundary", True))))
    bare = mesh.extract_mesh(model, res, smooth=2)
    full = mesh.extract_mesh(model, res)
    assert bare.colors is None and same_mesh(bare, mesh.smooth_taubin(full, cell, 2, origin=lo))


def test_cli_smooth(true_density, tmp_path, capsys):
    from ngp_pl_amd import mesh
    from tests.test_meshfilter_gpu import read_ply
    model = make_model()
    res = 48
    slim = {"model." + k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt, out = str(tmp_path / "slim.ckpt"), str(tmp_path / "m.ply")
    torch.save(slim, ckpt)
    xyz = lambda verts, names: np.stack([verts[n] for n in names], 1)
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--smooth-iterations", "5", "--out", out]) == 0
    full = mesh.extract_mesh(model, res)
    want = mesh.extract_mesh(model, res, smooth=5)
    verts, faces = read_ply(out)
    assert np.array_equal(faces, full.faces.cpu().numpy())
    assert np.array_equal(bits(xyz(verts, "xyz")), bits(want.vertices)) and np.array_equal(bits(xyz(verts, ("nx", "ny", "nz"))), bits(want.normals))
    lo, hi = mesh._box(model)
    topo = mesh.mesh_topology(full, max((b - a) / (res - 1) for a, b in zip(lo, hi)), origin=lo)
    last = capsys.readouterr().out.strip().splitlines()[-1]
    assert last == "%s: %d vertices, %d faces, smoothed 5 pairs, %d of %d vertices free" % (out, len(verts), len(faces), topo.n_free, len(verts))
    assert 0 < topo.n_free <= len(verts)
    # the other flags, behind the component filter and the simplification
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--keep-largest", "1", "--simplify-voxels", "2", "--smooth-iterations", "3",
                      "--smooth-lambda", "0.6", "--smooth-mu", "-0.63", "--smooth-free-boundary", "--out", out]) == 0
    want = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, smooth=dict(iterations=3, lam=0.6, mu=-0.63, pin_boundary=False))
    verts, faces = read_ply(out)
    assert np.array_equal(faces, want.faces.cpu().numpy()) and np.array_equal(bits(xyz(verts, "xyz")), bits(want.vertices))
    last = capsys.readouterr().out.strip().splitlines()[-1]
    found = re.fullmatch(re.escape("%s: %d vertices, %d faces, " % (out, len(verts), len(faces)))
                         + r"\d+ components found, 1 kept, simplified \d+ -> (\d+) vertices, \d+ -> (\d+) faces, smoothed 3 pairs, (\d+) of (\d+) vertices free",
                         last)
    assert found and [int(x) for x in found.groups()] == [len(verts), len(faces), len(verts), len(verts)]
    # without the flag: the line and the mesh of before
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--out", out]) == 0
    verts, faces = read_ply(out)
    assert np.array_equal(faces, full.faces.cpu().numpy()) and np.array_equal(bits(xyz(verts, "xyz")), bits(full.vertices))
    assert np.array_equal(bits(xyz(verts, ("nx", "ny", "nz"))), bits(full.normals))
    assert capsys.readouterr().out.strip().splitlines()[-1] == "%s: %d vertices, %d faces" % (out, len(verts), len(faces))
