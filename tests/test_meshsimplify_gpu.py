"""GPU: the vertex clustering of libngp_meshsimplify.so, bit for bit against the numpy restatement
(tests/mesh_simplify_reference.py): labels, positions, normals and colours as bit patterns, faces and the three totals, on the
smallest inputs at which each mechanism can fail (block and wave edges, probing chains with high key bits, one heavy cluster,
duplicate faces, bad input, absent attributes, empty results), on marching-cubes meshes, twice and on a side stream, and through
extract_mesh(simplify_voxels=...) and the CLI.  The sums are integers and the means are single f64 expressions: nothing here has
a tolerance."""
import re

import numpy as np
import pytest
import torch

from tests import mc_reference as R
from tests import mesh_simplify_reference as SR
from tests import mesh_visibility_reference as VR

pytestmark = pytest.mark.gpu


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def to_mesh(v, f, n=None, c=None, device="cuda"):
    from ngp_pl_amd import mesh
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return mesh.Mesh(t(v), t(f), t(n), t(c))


def same_mesh(a, b):
    ok = torch.equal(a.faces, b.faces) and torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))
    for x, y in ((a.normals, b.normals), (a.colors, b.colors)):
        ok = ok and (x is None) == (y is None) and (x is None or torch.equal(x.view(torch.int32), y.view(torch.int32)))
    return ok


def check(v, f, cell, origin, n=None, c=None):
    """simplify_clusters, vertex_clusters and the totals against the restatement, exactly; returns the restatement's result."""
    from ngp_pl_amd import mesh
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)
    origin = np.asarray(origin, np.float32)
    wv, wf, wn, wc, wlabel, wclusters = SR.simplify(v, f, origin, np.float32(cell), n, c)
    m = to_mesh(v, f, n, c)
    vv, ff, extra = mesh._check_mesh(m)
    got, label, totals = mesh._simplify(vv, ff, extra, float(np.float32(cell)), origin.tolist())
    assert label.dtype == torch.int32 and np.array_equal(label.cpu().numpy(), wlabel), "%d labels differ" % (label.cpu().numpy() != wlabel).sum()
    assert totals == (len(wv), len(wf), wclusters)
    assert got.faces.dtype == torch.int32 and got.faces.shape == wf.shape and np.array_equal(got.faces.cpu().numpy(), wf)
    for name, a, w in (("vertices", got.vertices, wv), ("normals", got.normals, wn), ("colors", got.colors, wc)):
        assert (a is None) == (w is None), name
        if w is not None:
            assert a.dtype == torch.float32 and a.shape == w.shape, name
            assert np.array_equal(bits(a), bits(w)), "%s: %d words differ" % (name, (bits(a) != bits(w)).sum())
    # the public functions are the same calls
    assert same_mesh(mesh.simplify_clusters(m, float(np.float32(cell)), origin=origin.tolist()), got)
    assert torch.equal(mesh.vertex_clusters(m, float(np.float32(cell)), origin=torch.from_numpy(origin)), label)
    return wv, wf, wn, wc, wlabel, wclusters


def sheet(n_v, n_f, seed, w=37):
    """n_v jittered points of a w-wide sheet of unit spacing and n_f faces (j, j + 1, j + w) over them, indices modulo n_v."""
    g = np.random.RandomState(seed)
    i = np.arange(n_v)
    v = np.stack([i % w, i // w, np.zeros(n_v)], 1) + g.uniform(-0.4, 0.4, (n_v, 3))
    j = np.arange(n_f)
    f = np.stack([j % n_v, (j + 1) % n_v, (j + w) % n_v], 1)
    return v.astype(np.float32), f.astype(np.int32), g


@pytest.mark.parametrize("n", [63, 64, 65, 2047, 2048, 2049, 4097])
def test_block_and_wave_edges(n):
    v, f, g = sheet(n, n, n)
    nrm = g.normal(size=(n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    col = g.uniform(0, 1, (n, 3)).astype(np.float32)
    wv, wf, _, _, _, clusters = check(v, f, 2.3, (-1, -1, -1), nrm, col)
    assert 0 < len(wv) <= clusters < n and 0 < len(wf) < n
    # faces and vertices on different sides of a block edge
    v2, f2, _ = sheet(n, 2 * n - 1, n + 1)
    check(v2, f2, 1.7, (-1, -1, -1))


def test_many_singleton_clusters_with_high_key_bits():
    g = np.random.RandomState(5)
    n = 6000
    c = np.unique(g.randint(0, 1 << 20, (2 * n, 3)), axis=0)
    c = c[g.permutation(len(c))[:n]] + (1 << 20)                               # cells around 2^20 on every axis, below 2^21
    c[0], c[1] = (1 << 21) - 1, [(1 << 21) - 1, 1 << 20, 0]                     # the last cell of an axis
    v = (c + 0.5).astype(np.float32)                                          # 22 bits and a half: exact in f32
    assert np.array_equal(v.astype(np.float64), c + 0.5)
    j = np.arange(n)
    f = np.stack([j, (j + 1) % n, (j + 2) % n], 1).astype(np.int32)
    wv, wf, _, _, label, clusters = check(v, f, 1.0, (0, 0, 0))
    assert clusters == n and np.array_equal(label, j) and np.array_equal(wf, f) and np.array_equal(wv, v)
    # a smaller cell: the same cells are 2^21 and beyond, outside the grid; nothing survives
    out = check(v, f, 0.5, (0, 0, 0))
    assert (out[4] == -1).all() and out[5] == 0 and out[0].shape == (0, 3) and out[1].shape == (0, 3)


def test_one_heavy_cluster_and_a_light_neighbour():
    g = np.random.RandomState(6)
    n = 5000                                                                   # three blocks of 2048, 79 waves
    v = np.concatenate([g.uniform(0, 1, (n, 3)), [[1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.25, 0.25, 0.25]]]).astype(np.float32)
    nrm = g.normal(size=(n + 3, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    col = g.uniform(-0.1, 1.1, (n + 3, 3)).astype(np.float32)
    f = np.stack([g.permutation(n)[:400], np.full(400, n), np.full(400, n + 1)], 1).astype(np.int32)
    wv, wf, wn, wc, label, clusters = check(v, f, 1.0, (0, 0, 0), nrm, col)
    assert clusters == 3 and (label[:n] == 0).all() and label[n:].tolist() == [n, n + 1, 0]
    assert wf.tolist() == [[0, 1, 2]] and len(wv) == 3
    assert np.abs(wv[0] - 0.5).max() < 0.02 and np.abs(wc[0] - 0.5).max() < 0.03
    # heavy and light clusters mixed inside waves: runs of 1 to 40 vertices per cell
    runs = g.randint(1, 41, 300)
    cell_of = np.repeat(np.arange(300), runs)
    v2 = (np.stack([cell_of % 20, cell_of // 20, np.zeros(len(cell_of))], 1) + g.uniform(0, 1, (len(cell_of), 3))).astype(np.float32)
    j = np.arange(len(v2))
    f2 = np.stack([j, (j + 17) % len(v2), (j + 401) % len(v2)], 1).astype(np.int32)
    n2 = g.normal(size=v2.shape).astype(np.float32)
    check(v2, f2, 1.0, (0, 0, 0), n2, g.uniform(0, 1, v2.shape).astype(np.float32))


def test_duplicate_faces_keep_exactly_the_lowest_index():
    g = np.random.RandomState(7)
    per = 12
    corners = np.array([[0.5, 0.5, 0.5], [3.5, 0.5, 0.5], [0.5, 3.5, 0.5]])
    tri = np.concatenate([corners[k] + g.uniform(-0.4, 0.4, (per, 3)) for k in range(3)])          # 12 vertices in each of three cells
    strip = np.stack([np.arange(3100) + 10.5, np.full(3100, 0.5), np.full(3100, 0.5)], 1)           # singletons
    v = np.concatenate([tri, strip]).astype(np.float32)
    faces = []
    for j in range(3000):
        abc = [g.randint(per), per + g.randint(per), 2 * per + g.randint(per)]
        faces.append(list(g.permutation(abc)))                                                      # any rotation, either orientation
        faces.append([3 * per + j, 3 * per + j + 1, 3 * per + j + 2])                               # a distinct face in between
    f = np.array(faces, np.int32)
    wv, wf, _, _, label, _ = check(v, f, 1.0, (0, 0, 0))
    group = {0, per, 2 * per}
    assert set(label[f[0]].tolist()) == group
    in_group = [i for i, face in enumerate(wf.tolist()) if set(face) <= {0, 1, 2}]
    assert in_group == [0] and wf[0].tolist() == [sorted(group).index(x) for x in label[f[0]].tolist()]     # its own orientation
    assert len(wf) == 3001
    # the group's first face late in the input, behind faces that do not survive
    f2 = np.concatenate([np.array([[0, 1, 2 * per]] * 70, np.int32), f[::-1]])
    check(v, f2, 1.0, (0, 0, 0))


@pytest.fixture(scope="module")
def sphere48():
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, 48, dtype=np.float32)] * 3, indexing="ij")
    v, f, n, _ = R.marching_cubes((np.float32(0.8) - np.sqrt(x * x + y * y + z * z)).astype(np.float32), 0.0, (-1, -1, -1), (1, 1, 1))
    return v, f, n, (0.5 * (v + 1)).astype(np.float32)


@pytest.fixture(scope="module")
def shells48():
    v, f, n, _ = R.marching_cubes(VR.shells_volume((48, 48, 48)), 0.0, (0, 0, 0), (1, 1, 1))
    return v, f, n, v.copy()


def test_bad_input_faults_nothing_and_matches(sphere48):
    v, f, n, c = [a.copy() for a in sphere48]
    g = np.random.RandomState(8)
    n_v = len(v)
    nan, inf = np.float32("nan"), np.float32("inf")
    rows = g.permutation(n_v)[:400]
    for k, bad in enumerate((nan, inf, -inf, np.float32(-1.5), np.float32(3e5), np.float32(3e38))):
        v[rows[60 * k:60 * k + 60], g.randint(0, 3, 60)] = bad                 # 3e5 / cell is beyond 2^21 cells, -1.5 below the origin
    n[rows[360:380], 0] = nan
    n[rows[370:390], 1] = inf
    c[rows[380:400], 2] = nan
    c[rows[385:400], 0] = -inf
    fr = g.permutation(len(f))[:300]
    for k, bad in enumerate((-1, n_v, 2 ** 31 - 1, -2 ** 31, n_v + 7)):
        f[fr[60 * k:60 * k + 60], g.randint(0, 3, 60)] = bad
    h = 2.0 / 47
    out = check(v, f, 2 * h, (-1, -1, -1), n, c)
    assert (out[4] == -1).sum() >= 300 and 0 < len(out[1]) < len(f)
    # a NaN origin: every vertex is outside the grid
    none = check(v, f, 2 * h, (nan, -1, -1), n, c)
    assert (none[4] == -1).all() and none[0].shape == (0, 3) and none[5] == 0


@pytest.mark.parametrize("with_normals", [False, True])
@pytest.mark.parametrize("with_colors", [False, True])
def test_null_attributes(with_normals, with_colors):
    v, f, g = sheet(700, 900, 9)
    n = g.normal(size=v.shape).astype(np.float32) if with_normals else None
    c = g.uniform(0, 1, v.shape).astype(np.float32) if with_colors else None
    out = check(v, f, 2.0, (-1, -1, -1), n, c)
    assert (out[2] is not None) == with_normals and (out[3] is not None) == with_colors


def test_empty_meshes_and_nothing_surviving():
    from ngp_pl_amd import mesh
    v, f, g = sheet(300, 400, 10)
    z3, zi = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    for m in (to_mesh(z3, zi), to_mesh(z3, zi, z3, z3), to_mesh(z3, f)):        # no vertices (faces or not): nothing is launched
        e = mesh.simplify_clusters(m, 0.5)
        assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3) and e.faces.dtype == torch.int32
        assert (e.normals is None) == (m.normals is None) and (e.colors is None) == (m.colors is None)
        assert mesh.vertex_clusters(m, 0.5).shape == (0,)
    out = check(v, zi, 2.0, (-1, -1, -1), v)                                   # vertices and no faces: clusters, no output
    assert out[5] > 0 and out[0].shape == (0, 3) and out[2].shape == (0, 3)
    out = check(v, f, 1000.0, (-1, -1, -1), v, v)                              # one cell holds everything: no face survives
    assert out[5] == 1 and (out[4] == 0).all() and out[0].shape == (0, 3) and out[1].shape == (0, 3) and out[3].shape == (0, 3)
    e = mesh.simplify_clusters(to_mesh(v, f, v, None), 1000.0)                  # origin = the minimum, taken on the device
    assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3) and e.normals.shape == (0, 3) and e.colors is None


@pytest.mark.parametrize("K", [2, 3, 4.5])
@pytest.mark.parametrize("scene", ["sphere", "shells"])
def test_marching_cubes_meshes(scene, K, sphere48, shells48):
    from ngp_pl_amd import mesh
    v, f, n, c = sphere48 if scene == "sphere" else shells48
    lo = -1.0 if scene == "sphere" else 0.0
    h = (1.0 - lo) / 47
    wv, wf, _, _, label, _ = check(v, f, K * h, (lo, lo, lo), n, c)
    assert 0 < len(wv) < len(v) / 2 and 0 < len(wf) < len(f) / 2
    # origin=None is the vertices' minimum, taken on the device
    m = to_mesh(v, f, n, c)
    cell = float(np.float32(K * h))
    got = mesh.simplify_clusters(m, cell)
    want = SR.simplify(v, f, v.min(0), np.float32(cell), n, c)
    assert np.array_equal(got.faces.cpu().numpy(), want[1])
    for a, w in ((got.vertices, want[0]), (got.normals, want[2]), (got.colors, want[3])):
        assert np.array_equal(bits(a), bits(w))
    # vertex_clusters against simplify_clusters: the faces, relabelled, are the clusters' faces
    lab = mesh.vertex_clusters(m, cell).cpu().numpy()
    assert np.array_equal(lab, want[4])
    used = np.unique(lab[f][(lab[f][:, 0] != lab[f][:, 1]) & (lab[f][:, 1] != lab[f][:, 2]) & (lab[f][:, 0] != lab[f][:, 2])])
    assert got.vertices.shape[0] == len(used)
    assert set(map(tuple, np.sort(used[got.faces.cpu().numpy()], 1).tolist())) <= set(map(tuple, np.sort(lab[f], 1).tolist()))


def test_two_runs_and_a_side_stream_are_bit_identical(shells48):
    from ngp_pl_amd import mesh
    v, f, n, c = shells48
    m = to_mesh(v, f, n, c)
    cell = 3.0 / 47
    a, b = [mesh.simplify_clusters(m, cell, origin=(0.0, 0.0, 0.0)) for _ in range(2)]
    assert a.faces.shape[0] > 0 and same_mesh(a, b)
    la, lb = [mesh.vertex_clusters(m, cell, origin=(0.0, 0.0, 0.0)) for _ in range(2)]
    assert torch.equal(la, lb)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = mesh.simplify_clusters(m, cell, origin=(0.0, 0.0, 0.0))
        lx = mesh.vertex_clusters(m, cell, origin=(0.0, 0.0, 0.0))
    side.synchronize()
    assert same_mesh(a, x) and torch.equal(la, lx)


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
    plain = mesh.extract_mesh(model, res, keep_largest=1, colors=True)
    none = mesh.extract_mesh(model, res, keep_largest=1, colors=True, simplify_voxels=None)
    assert same_mesh(plain, none)                                              # without the option: today's output
    got = mesh.extract_mesh(model, res, simplify_voxels=3, keep_largest=1, colors=True)
    lo, hi = mesh._box(model)
    cell = 3.0 * max((b - a) / (res - 1) for a, b in zip(lo, hi))
    want = mesh.simplify_clusters(mesh.Mesh(plain.vertices, plain.faces, plain.normals), cell, origin=lo)
    assert 0 < want.faces.shape[0] < plain.faces.shape[0] / 2 and 0 < want.vertices.shape[0] < plain.vertices.shape[0] / 2
    assert same_mesh(mesh.Mesh(got.vertices, got.faces, got.normals), want)
    # colours: evaluated on the simplified vertices, along minus the averaged normals
    assert got.colors.shape == got.vertices.shape
    assert torch.allclose(got.colors, mesh.vertex_colors(model, want.vertices, want.normals), atol=1e-6)
    bare = mesh.extract_mesh(model, res, simplify_voxels=3, keep_largest=1)
    assert bare.colors is None and same_mesh(bare, want)


def test_cli_simplify_voxels(true_density, tmp_path, capsys):
    from ngp_pl_amd import mesh
    from tests.test_meshfilter_gpu import read_ply
    model = make_model()
    res = 48
    slim = {"model." + k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt, out = str(tmp_path / "slim.ckpt"), str(tmp_path / "m.ply")
    torch.save(slim, ckpt)
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--simplify-voxels", "2.5", "--out", out]) == 0
    full = mesh.extract_mesh(model, res)
    want = mesh.extract_mesh(model, res, simplify_voxels=2.5)
    verts, faces = read_ply(out)
    assert 0 < len(faces) < full.faces.shape[0] and np.array_equal(faces, want.faces.cpu().numpy())
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), want.vertices.cpu().numpy())
    last = capsys.readouterr().out.strip().splitlines()[-1]
    assert last == "%s: %d vertices, %d faces, simplified %d -> %d vertices, %d -> %d faces" % (
        out, len(verts), len(faces), full.vertices.shape[0], len(verts), full.faces.shape[0], len(faces))
    # behind the component filter
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--keep-largest", "1", "--simplify-voxels", "2", "--out", out]) == 0
    verts, faces = read_ply(out)
    last = capsys.readouterr().out.strip().splitlines()[-1]
    found = re.fullmatch(re.escape("%s: %d vertices, %d faces, " % (out, len(verts), len(faces)))
                         + r"\d+ components found, 1 kept, simplified (\d+) -> (\d+) vertices, (\d+) -> (\d+) faces", last)
    assert found and int(found.group(2)) == len(verts) and int(found.group(4)) == len(faces)
    # without the flag: the line and the mesh of before
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--out", out]) == 0
    verts, faces = read_ply(out)
    assert np.array_equal(faces, full.faces.cpu().numpy())
    assert capsys.readouterr().out.strip().splitlines()[-1] == "%s: %d vertices, %d faces" % (out, len(verts), len(faces))
