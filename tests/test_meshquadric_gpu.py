"""GPU: the quadric placement of libngp_meshquadric.so against the numpy restatement (tests/mesh_quadric_reference.py): the 14
int64 sums exactly, positions and states bit for bit, the three totals, on the smallest inputs at which each mechanism can fail
(block and wave edges, one heavy cluster beside a light one, singleton clusters with high key bits, bad input, no faces, nothing at
all), on the box, sphere and wedge of tests/test_meshquadric_cpu.py, twice, on a side stream and with the faces permuted, and
through simplify_clusters(placement="quadric"), extract_mesh(simplify_placement="quadric") and the CLI.  Nothing compared with the
restatement has a tolerance; the geometric bounds are the issue's: cell / 256 on the box, a strictly smaller radial error on the
sphere."""
import numpy as np
import pytest
import torch

from tests import mesh_quadric_reference as QR
from tests import test_meshquadric_cpu as G
from tests.test_meshsimplify_gpu import bits, make_model, same_mesh, to_mesh, true_density  # noqa: F401  (true_density is a fixture)

pytestmark = pytest.mark.gpu


def device_placement(v, f, cell, origin, label=None):
    """_cluster (unless `label` is given), _place and the sums hook -> positions, state, label, sums, totals as numpy arrays."""
    from ngp_pl_amd import _meshquadric_lib as ql
    from ngp_pl_amd import mesh
    m = to_mesh(v, f)
    vv, ff, _ = mesh._check_mesh(m)
    n_v = vv.shape[0]
    lab, _, _, o = mesh._cluster(vv, (None, None), float(cell), [float(x) for x in origin], 0)
    if label is not None:
        lab = torch.from_numpy(np.ascontiguousarray(label, np.int32)).cuda()
    positions, state, totals, (ws, ws_bytes) = mesh._place(vv, ff, lab, float(cell), o)
    sums = torch.full((n_v, QR.SUMS), -7, dtype=torch.int64, device="cuda")
    ql.call("ngp_meshquadric_sums", ql.ptr(lab), n_v, ql.ptr(ws), ws_bytes, ql.ptr(sums), ql.stream())
    return positions.cpu().numpy(), state.cpu().numpy(), lab.cpu().numpy(), sums.cpu().numpy(), totals.cpu().numpy()


def check(v, f, cell, origin, label=None, public=True):
    """Everything the library computes against the restatement, exactly; returns the restatement's result."""
    from ngp_pl_amd import mesh
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    origin, cell = np.asarray(origin, np.float32), np.float32(cell)
    want = QR.cluster_placement(v, f, origin, cell, label)
    wpos, wstate, wlabel, wsums, wtotals = want
    pos, state, lab, sums, totals = device_placement(v, f, cell, origin, label)
    assert np.array_equal(lab, wlabel)
    wexp = QR.exported_sums(wsums, wlabel)
    assert sums.dtype == np.int64 and np.array_equal(sums, wexp), "%d sums differ in columns %s" % (
        (sums != wexp).sum(), sorted(set(np.nonzero(sums != wexp)[1].tolist())))
    assert state.dtype == np.uint8 and np.array_equal(state, wstate), "%d states differ" % (state != wstate).sum()
    assert np.array_equal(totals, wtotals)
    assert pos.dtype == np.float32 and np.array_equal(bits(pos), bits(wpos)), "%d words differ" % (bits(pos) != bits(wpos)).sum()
    if public and label is None:
        m = to_mesh(v, f)
        p, s, l = mesh.cluster_placement(m, float(cell), origin=origin.tolist())
        assert np.array_equal(bits(p), bits(wpos)) and np.array_equal(s.cpu().numpy(), wstate) and np.array_equal(l.cpu().numpy(), wlabel)
        wq = QR.simplify(v, f, origin, cell, placement="quadric")
        got = mesh.simplify_clusters(m, float(cell), origin=origin.tolist(), placement="quadric")
        mean = mesh.simplify_clusters(m, float(cell), origin=origin.tolist())
        assert got.vertices.shape == wq[0].shape and np.array_equal(bits(got.vertices), bits(wq[0]))
        assert torch.equal(got.faces, mean.faces) and np.array_equal(got.faces.cpu().numpy(), wq[1])
    return want


@pytest.mark.parametrize("n", [63, 64, 65, 2047, 2048, 2049, 4097])
def test_block_and_wave_edges(n):
    v, f, _ = G.sheet(n, n, n)
    _, state, _, sums, totals = check(v, f, 2.3, (-1, -1, -1))
    assert totals[0] > 0 and totals.sum() == (state != 0).sum() and sums[:, 13].sum() > 0
    # corners and vertices on different sides of a block edge: 3 (2 n - 1) corners
    v2, f2, _ = G.sheet(n, 2 * n - 1, n + 1)
    check(v2, f2, 1.7, (-1, -1, -1))


def test_one_heavy_cluster_and_a_light_neighbour():
    g = np.random.RandomState(6)
    n = 1500
    v = np.concatenate([g.uniform(0, 1, (n, 3)), [[1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.25, 0.25, 0.25]]]).astype(np.float32)
    heavy = np.stack([g.randint(0, n, 3000), g.randint(0, n, 3000), g.randint(0, n, 3000)], 1)        # some 9000 corners on label 0
    light = np.stack([g.permutation(n)[:40], np.full(40, n), np.full(40, n + 1)], 1)
    f = np.concatenate([heavy, light, [[n, n + 1, n + 2]]]).astype(np.int32)
    _, state, label, sums, _ = check(v, f[g.permutation(len(f))], 1.0, (0, 0, 0))
    assert (label[:n] == 0).all() and label[n:].tolist() == [n, n + 1, 0] and sums[0, 0] == n + 1
    assert sums[0, 13] > 3000 * (1 << 24) * 0.05 and 0 < sums[n, 13] < sums[0, 13] / 20
    # heavy and light clusters mixed inside waves: runs of 1 to 40 vertices per cell
    runs = g.randint(1, 41, 300)
    cell_of = np.repeat(np.arange(300), runs)
    v2 = (np.stack([cell_of % 20, cell_of // 20, np.zeros(len(cell_of))], 1) + g.uniform(0, 1, (len(cell_of), 3))).astype(np.float32)
    j = np.arange(len(v2))
    f2 = np.stack([j, (j + 1) % len(v2), (j + 2) % len(v2)], 1).astype(np.int32)
    check(v2, f2, 1.0, (0, 0, 0))


def test_many_singleton_clusters_with_high_key_bits():
    g = np.random.RandomState(5)
    n = 6000
    c = np.unique(g.randint(0, 1 << 20, (2 * n, 3)), axis=0)
    c = c[g.permutation(len(c))[:n]] + (1 << 20)                               # cells around 2^20 on every axis, below 2^21
    c[0], c[1] = (1 << 21) - 1, [(1 << 21) - 1, 1 << 20, 0]                     # the last cell of an axis
    v = (c + 0.5).astype(np.float32)
    j = np.arange(n)
    f = np.stack([j, (j + 1) % n, (j + 2) % n], 1).astype(np.int32)
    pos, state, label, sums, totals = check(v, f, 1.0, (0, 0, 0))
    assert np.array_equal(label, j) and (sums[:, 0] == 1).all() and (sums[:, 13] == 3 * 16 << 24).all()       # every face at W_MAX
    assert totals.sum() == n and totals[0] > 0
    # a smaller cell: the same cells are 2^21 and beyond, outside the grid; nothing is a leader
    pos, state, label, sums, totals = check(v, f, 0.5, (0, 0, 0))
    assert (label == -1).all() and (state == 0).all() and (sums == 0).all() and (totals == 0).all()


@pytest.mark.parametrize("n,cell", G.BOX_CASES)
def test_box_vertices_land_on_the_surface(n, cell):
    from ngp_pl_amd import mesh
    v, f = G.box(n)
    _, _, _, _, totals = check(v, f, cell, (0, 0, 0))
    assert totals[1] == 0 and totals[2] == 0                                   # no MEAN_OUTSIDE (and no cluster without faces)
    m = to_mesh(v, f)
    c32 = float(np.float32(cell))
    q = mesh.simplify_clusters(m, c32, origin=(0.0, 0.0, 0.0), placement="quadric")
    a = mesh.simplify_clusters(m, c32, origin=(0.0, 0.0, 0.0), placement="mean")
    dq, da = G.box_distance(q.vertices.cpu().numpy()) / cell, G.box_distance(a.vertices.cpu().numpy()) / cell
    print("box n=%d cell=%g: quadric worst %.3e cell, mean worst %.3e cell, %d vertices" % (n, cell, dq.max(), da.max(), len(dq)))
    assert len(dq) == len(da) > 0 and torch.equal(q.faces, a.faces)
    assert dq.max() <= 1.0 / 256
    assert da.max() >= 1.0 / 8


@pytest.fixture(scope="module")
def sphere48():
    return G.sphere48()


@pytest.mark.parametrize("K", [2, 3, 4.5])
def test_sphere_radial_error_drops(sphere48, K):
    from ngp_pl_amd import mesh
    v, f = sphere48
    cell = float(np.float32(K * 2.0 / 47))
    _, state, _, _, totals = check(v, f, cell, (-1, -1, -1))
    m = to_mesh(v, f)
    q = mesh.simplify_clusters(m, cell, origin=(-1.0, -1.0, -1.0), placement="quadric")
    a = mesh.simplify_clusters(m, cell, origin=(-1.0, -1.0, -1.0), placement="mean")
    eq, ea = G.radial_error(q.vertices.cpu().numpy()), G.radial_error(a.vertices.cpu().numpy())
    print("sphere K=%g: quadric %.3e, mean %.3e, totals %s" % (K, eq, ea, totals.tolist()))
    assert eq < ea
    assert totals[2] * 8 <= totals.sum()


def test_wedge_falls_back_to_the_mean():
    from ngp_pl_amd import mesh
    v, f = G.wedge(0.1)
    _, state, label, _, totals = check(v, f, G.WEDGE_CELL, G.WEDGE_ORIGIN)
    assert totals.tolist() == [0, 0, 2]
    # with a third cluster and one small face that reaches all three, the simplifier emits them: the same bits
    v3 = np.concatenate([v, np.float32([[2.98, 1.02, 0.0]])])
    near = [int(np.abs(v[:81] - np.float32(p)).sum(1).argmin()) for p in ([2.8875, 0.9, 0.28875], [3.1125, 0.9, 0.31125])]
    f3 = np.concatenate([f, np.int32([[near[0], near[1], len(v)]])])
    _, state3, label3, _, totals3 = check(v3, f3, G.WEDGE_CELL, G.WEDGE_ORIGIN)
    assert totals3.tolist() == [1, 0, 2] and len(np.unique(label3)) == 3
    m = to_mesh(v3, f3)
    q = mesh.simplify_clusters(m, G.WEDGE_CELL, origin=G.WEDGE_ORIGIN, placement="quadric")
    a = mesh.simplify_clusters(m, G.WEDGE_CELL, origin=G.WEDGE_ORIGIN, placement="mean")
    assert q.vertices.shape == (3, 3) and torch.equal(q.faces, a.faces)
    outside = torch.from_numpy(state3[np.unique(label3)] == QR.MEAN_OUTSIDE).cuda()
    assert outside.sum() == 2 and torch.equal(q.vertices[outside].view(torch.int32), a.vertices[outside].view(torch.int32))
    # a shallower wedge: both states occur
    v, f = G.wedge(0.02)
    _, _, _, _, totals = check(v, f, G.WEDGE_CELL, G.WEDGE_ORIGIN)
    assert totals[0] >= 1 and totals[2] >= 1 and totals.sum() == 2


def test_bad_input_faults_nothing_and_matches(sphere48):
    v, f = [a.copy() for a in sphere48]
    g = np.random.RandomState(8)
    n_v = len(v)
    nan, inf = np.float32("nan"), np.float32("inf")
    rows = g.permutation(n_v)[:360]
    for k, bad in enumerate((nan, inf, -inf, np.float32(-1.5), np.float32(3e5), np.float32(3e38))):
        v[rows[60 * k:60 * k + 60], g.randint(0, 3, 60)] = bad                 # 3e5 / cell is beyond 2^21 cells, -1.5 below the origin
    fr = g.permutation(len(f))[:500]
    for k, bad in enumerate((-1, n_v, 2 ** 31 - 1, -2 ** 31, n_v + 7)):
        f[fr[60 * k:60 * k + 60], g.randint(0, 3, 60)] = bad                   # indices out of range
    f[fr[300:360], 1] = f[fr[300:360], 0]                                      # repeated indices
    f[fr[360:400]] = f[fr[360:400], :1]                                        # one vertex three times
    v[f[fr[400:430], 1]] = v[f[fr[400:430], 0]]                                # zero-area faces of distinct indices
    mid = f[fr[430:460]]
    ok = ((mid >= 0) & (mid < n_v)).all(1)
    v[mid[ok, 2]] = (0.5 * (v[mid[ok, 0]].astype(np.float64) + v[mid[ok, 1]])).astype(np.float32)      # (nearly) collinear
    cell = 2 * 2.0 / 47
    pos, state, label, sums, totals = check(v, f, cell, (-1, -1, -1))
    assert (label == -1).sum() >= 300 and totals[0] > 0 and totals.sum() == (label == np.arange(n_v)).sum()
    # labels of -1 and labels that are no vertex, where the simplifier gave a cluster: nothing is read through them
    bad_label = label.copy()
    hit = g.permutation(n_v)[:300]
    bad_label[hit[:150]] = -1
    bad_label[hit[150:200]] = n_v
    bad_label[hit[200:250]] = 2 ** 31 - 1
    bad_label[hit[250:300]] = -2 ** 31
    out = check(v, f, cell, (-1, -1, -1), label=bad_label)
    assert 0 < out[4].sum() < totals.sum()
    # a NaN origin: every vertex is outside the grid
    none = check(v, f, cell, (nan, -1, -1))
    assert (none[2] == -1).all() and (none[1] == 0).all() and (none[3] == 0).all() and (none[4] == 0).all()


def test_empty_meshes_launch_nothing():
    from ngp_pl_amd import mesh
    v, f, _ = G.sheet(300, 400, 10)
    z3, zi = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    for m in (to_mesh(z3, zi), to_mesh(z3, f)):                                # no vertices, faces or not
        p, s, l = mesh.cluster_placement(m, 0.5)
        assert p.shape == (0, 3) and s.shape == (0,) and l.shape == (0,) and s.dtype == torch.uint8 and l.dtype == torch.int32
        e = mesh.simplify_clusters(m, 0.5, placement="quadric")
        assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3) and e.faces.dtype == torch.int32
    # one cell holds everything: no face survives
    e = mesh.simplify_clusters(to_mesh(v, f, v, None), 1000.0, placement="quadric")
    assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3) and e.normals.shape == (0, 3) and e.colors is None


def test_a_mesh_without_faces_gives_the_mean():
    from ngp_pl_amd import mesh
    v, f, _ = G.sheet(700, 900, 9)
    zi = np.zeros((0, 3), np.int32)
    pos, state, label, sums, totals = check(v, zi, 2.0, (-1, -1, -1))
    lead = label == np.arange(len(v))
    assert lead.sum() > 50 and (state[lead] == QR.MEAN_NO_FACES).all() and totals.tolist() == [0, lead.sum(), 0] and (sums[:, 4:] == 0).all()
    # bitwise the simplifier's: with the faces, the simplifier emits the clusters they reference
    a = mesh.simplify_clusters(to_mesh(v, f), 2.0, origin=(-1.0, -1.0, -1.0))
    lab = label[f]
    used = np.unique(lab[(lab[:, 0] != lab[:, 1]) & (lab[:, 1] != lab[:, 2]) & (lab[:, 0] != lab[:, 2])])
    assert len(used) == a.vertices.shape[0] > 20 and np.array_equal(bits(pos[used]), bits(a.vertices))
    # the default placement is the mean, bit for bit, and loads nothing new
    b = mesh.simplify_clusters(to_mesh(v, f), 2.0, origin=(-1.0, -1.0, -1.0), placement="mean")
    assert same_mesh(a, b)


def test_reproducible_on_a_side_stream_and_under_a_permutation_of_the_faces(sphere48):
    from ngp_pl_amd import mesh
    v, f = sphere48
    g = np.random.RandomState(11)
    cell, origin = 3 * 2.0 / 47, (-1.0, -1.0, -1.0)
    m = to_mesh(v, f)
    runs = [mesh.cluster_placement(m, cell, origin=origin) for _ in range(2)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        runs.append(mesh.cluster_placement(m, cell, origin=origin))
        sq = mesh.simplify_clusters(m, cell, origin=origin, placement="quadric")
    side.synchronize()
    shuffled = f[g.permutation(len(f))]
    shuffled = np.where(g.rand(len(f), 1) < 0.5, shuffled[:, ::-1], shuffled)                          # and half of them reversed
    runs.append(mesh.cluster_placement(to_mesh(v, np.ascontiguousarray(shuffled)), cell, origin=origin))
    p0, s0, l0 = runs[0]
    assert (s0 == QR.QUADRIC).sum() > 500
    for p, s, l in runs[1:]:
        assert torch.equal(p.view(torch.int32), p0.view(torch.int32)) and torch.equal(s, s0) and torch.equal(l, l0)
    assert same_mesh(sq, mesh.simplify_clusters(m, cell, origin=origin, placement="quadric"))


def test_extract_mesh_chain(true_density):  # noqa: F811
    from ngp_pl_amd import mesh
    model = make_model()
    res = 48
    plain = mesh.extract_mesh(model, res, keep_largest=1)
    lo, hi = mesh._box(model)
    cell = 2.0 * max((b - a) / (res - 1) for a, b in zip(lo, hi))
    want = mesh.simplify_clusters(mesh.Mesh(plain.vertices, plain.faces, plain.normals), cell, origin=lo, placement="quadric")
    got = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, simplify_placement="quadric")
    mean = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2)
    assert 0 < want.faces.shape[0] < plain.faces.shape[0] and same_mesh(got, want)
    assert torch.equal(got.faces, mean.faces) and torch.equal(got.normals.view(torch.int32), mean.normals.view(torch.int32))
    assert got.vertices.shape == mean.vertices.shape and not torch.equal(got.vertices, mean.vertices)
    assert same_mesh(mean, mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, simplify_placement="mean"))
    # no vertex leaves its cell by more than half a cell
    assert ((got.vertices - mean.vertices).abs().max() <= 1.5 * cell).item()
    colored = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, simplify_placement="quadric", colors=True)
    assert torch.equal(colored.vertices, got.vertices) and colored.colors.shape == got.vertices.shape


def test_cli_simplify_placement(true_density, tmp_path, capsys):  # noqa: F811
    from ngp_pl_amd import mesh
    from tests.test_meshfilter_gpu import read_ply
    model = make_model()
    res = 48
    slim = {"model." + k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt, out = str(tmp_path / "slim.ckpt"), str(tmp_path / "m.ply")
    torch.save(slim, ckpt)
    argv = ["--ckpt", ckpt, "--resolution", str(res), "--simplify-voxels", "2", "--out", out]
    assert mesh.main(argv + ["--simplify-placement", "quadric"]) == 0
    full = mesh.extract_mesh(model, res)
    want = mesh.extract_mesh(model, res, simplify_voxels=2, simplify_placement="quadric")
    verts, faces = read_ply(out)
    assert 0 < len(faces) < full.faces.shape[0] and np.array_equal(faces, want.faces.cpu().numpy())
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), want.vertices.cpu().numpy())
    last = capsys.readouterr().out.strip().splitlines()[-1]
    assert last == "%s: %d vertices, %d faces, simplified %d -> %d vertices, %d -> %d faces" % (
        out, len(verts), len(faces), full.vertices.shape[0], len(verts), full.faces.shape[0], len(faces))
    # "mean" on the command line is the default's PLY
    assert mesh.main(argv + ["--simplify-placement", "mean"]) == 0
    mean = mesh.extract_mesh(model, res, simplify_voxels=2)
    verts, faces2 = read_ply(out)
    assert np.array_equal(faces2, faces) and np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), mean.vertices.cpu().numpy())
