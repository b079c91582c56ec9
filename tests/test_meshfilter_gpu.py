"""GPU: connected components and component filtering of libngp_meshfilter.so, exact against the numpy restatement
(tests/mesh_components_reference.py) on marching-cubes meshes and on a soup built to stress the union-find; the filter's
invariants, determinism, the model path (extract_mesh with filter options, colours after the filter) and the CLI."""
import numpy as np
import pytest
import torch

from tests import mc_reference as R
from tests import mesh_components_reference as CR

pytestmark = pytest.mark.gpu


def smooth_volume(shape, seed, blobs=10):
    """Sum of random narrow Gaussian blobs: a smooth field whose iso-surface has several components."""
    g = np.random.RandomState(seed)
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.linspace(0, 1, nz), np.linspace(0, 1, ny), np.linspace(0, 1, nx), indexing="ij")
    v = np.zeros(shape)
    for _ in range(blobs):
        c, s, a = g.rand(3), 0.04 + 0.08 * g.rand(), 0.5 + g.rand()
        v += a * np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * s * s))
    return v.astype(np.float32)


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def to_mesh(v, f, n=None, c=None, device="cuda"):
    from ngp_pl_amd import mesh
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return mesh.Mesh(t(v), t(f), t(n), t(c))


def check_components(m, v, f):
    """connected_components against the restatement, every output exactly; returns the restatement's table."""
    from ngp_pl_amd import mesh
    got, want = mesh.connected_components(m), CR.Components(f, len(v))
    assert got.vertex_label.dtype == torch.int32 and got.face_label.dtype == torch.int32
    assert got.labels.dtype == torch.int32 and got.faces_per_component.dtype == torch.int64
    assert np.array_equal(got.vertex_label.cpu().numpy(), want.vertex_label)
    assert np.array_equal(got.face_label.cpu().numpy(), want.face_label)
    assert np.array_equal(got.labels.cpu().numpy(), want.labels)
    assert np.array_equal(got.faces_per_component.cpu().numpy(), want.faces_per_component)
    assert got.n_components == want.n_components == len(want.labels)          # the device counter and the table agree
    return want


def check_filter(m, v, f, n, c, **opts):
    from ngp_pl_amd import mesh
    got = mesh.filter_components(m, **opts)
    wv, wf, wn, wc = CR.filter_components(v, f, n, c, **opts)
    assert got.faces.dtype == torch.int32 and got.faces.shape == wf.shape and np.array_equal(got.faces.cpu().numpy(), wf)
    assert got.vertices.shape == wv.shape and np.array_equal(bits(got.vertices), bits(wv))
    for a, w in ((got.normals, wn), (got.colors, wc)):
        assert (a is None) == (w is None)
        if w is not None:
            assert a.shape == w.shape and np.array_equal(bits(a), bits(w))
    return got


@pytest.mark.parametrize("shape,seed", [((48, 48, 48), 0), ((72, 56, 40), 1), ((128, 128, 128), 2)])
def test_marching_cubes_meshes_exact_against_the_restatement(shape, seed):
    """(nz, ny, nx) = (72, 56, 40) is the non-cubic lattice.  The mesh is the GPU's own marching cubes of the volume."""
    from ngp_pl_amd import mesh
    vol = smooth_volume(shape, seed)
    m = mesh.marching_cubes(torch.from_numpy(vol).cuda(), 0.6, ((0, 0, 0), (1, 1, 1)))
    v, f, n = m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.normals.cpu().numpy()
    assert len(f) > 1000
    want = check_components(m, v, f)
    assert want.n_components >= 3, want.n_components
    c = np.random.RandomState(seed).rand(len(v), 3).astype(np.float32)
    mc = to_mesh(v, f, n, c)
    mid = int(np.sort(want.faces_per_component)[want.n_components // 2])
    for opts in (dict(keep_largest=1), dict(keep_largest=2), dict(min_faces=mid), dict(min_faces=mid + 1), dict(keep_largest=2, min_faces=mid)):
        check_filter(mc, v, f, n, c, **opts)
    one = check_filter(m, v, f, n, None, keep_largest=1)
    assert mesh.connected_components(one).n_components == 1


def noise_volume(n, seed):
    g = np.random.RandomState(seed)
    vol = g.rand(n, n, n).astype(np.float32)
    vol[[0, -1]] = 0
    vol[:, [0, -1]] = 0
    vol[:, :, [0, -1]] = 0
    return vol


def test_bordered_noise_thousands_of_tiny_components():
    from ngp_pl_amd import mesh
    vol = noise_volume(64, 5)
    assert len(np.unique(R.cube_indices(vol, 0.5))) == 256                   # every cube case occurs
    # a high iso-level leaves isolated specks, 0.5 one big tangle plus specks
    for thr in (0.5, 0.85):
        m = mesh.marching_cubes(torch.from_numpy(vol).cuda(), thr, ((0, 0, 0), (1, 1, 1)))
        v, f, n = m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.normals.cpu().numpy()
        want = check_components(m, v, f)
        assert want.n_components > 1000, want.n_components
        check_filter(m, v, f, n, None, keep_largest=1)
        check_filter(m, v, f, n, None, min_faces=9)
        check_filter(m, v, f, n, None, keep_largest=500, min_faces=8)       # hundreds of ties at 8 faces


def strip_soup(n_strip_faces=200_000, seed=0, shuffle_faces=False):
    """Vertex layout: tetrahedron A (4 faces) | isolated | a triangle strip of n_strip_faces faces whose numbering runs backwards
    along the strip, half of it shuffled | isolated | tetrahedron B (4 faces).  Run in face order the backwards numbering hooks
    each new root under the next, a chain as long as the strip, before the flatten pass."""
    g = np.random.RandomState(seed)
    n_s = n_strip_faces + 2
    ids = np.arange(n_s)[::-1].copy()
    sel = g.choice(n_s, n_s // 2, replace=False)
    ids[sel] = ids[g.permutation(sel)]
    iso = 700
    off = 4 + iso
    ids += off
    k = np.arange(n_strip_faces)
    strip = np.stack([ids[k], ids[k + 1], ids[k + 2]], 1)
    strip[1::2] = strip[1::2][:, [1, 0, 2]]
    tet = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
    n_v = off + n_s + iso + 4
    faces = np.concatenate([tet + (n_v - 4), strip[:1000], tet, strip[1000:]]).astype(np.int32)
    if shuffle_faces:
        faces = faces[g.permutation(len(faces))]
    # any bit pattern must survive the copy (NaN payloads, denormals, -0)
    attrs = [g.randint(-2 ** 31, 2 ** 31, (n_v, 3), dtype=np.int64).astype(np.int32).view(np.float32) for _ in range(3)]
    return attrs[0], faces, attrs[1], attrs[2]


@pytest.mark.parametrize("shuffle_faces", [False, True])
def test_strip_soup_deep_tree_isolated_vertices_and_ties(shuffle_faces):
    v, f, n, c = strip_soup(shuffle_faces=shuffle_faces)
    assert len(f) >= 200_000
    m = to_mesh(v, f, n, c)
    want = check_components(m, v, f)
    n_v = len(v)
    assert want.labels.tolist() == [0, 704, n_v - 4] and want.faces_per_component.tolist() == [4, 200_000, 4]
    assert (want.vertex_label[4:704] == np.arange(4, 704)).all()            # isolated vertices are their own components
    one = check_filter(m, v, f, n, c, keep_largest=1)
    assert one.faces.shape[0] == 200_000 and one.vertices.shape[0] == 200_002
    two = check_filter(m, v, f, n, c, keep_largest=2)                        # the tie between the tetrahedra goes to label 0
    assert two.vertices.shape[0] == 200_006 and np.array_equal(bits(two.vertices[:4]), bits(v[:4]))
    check_filter(m, v, f, n, c, keep_largest=3)                              # everything but the isolated vertices
    check_filter(m, v, f, n, c, min_faces=4)
    check_filter(m, v, f, n, c, min_faces=5)
    check_filter(m, v, f, n, c, keep_largest=2, min_faces=5)
    tets = check_filter(to_mesh(v, f), v, f, None, None, keep_largest=3, min_faces=4)
    assert tets.normals is None and tets.colors is None


def pair_soup(n_v=None, n_f=None):
    """Periods of nine vertices and three faces: two triangles that share an edge (vertices 0-3), an unreferenced vertex, a lone
    triangle (vertices 5-7), an unreferenced vertex.  Cut to n_f faces, or padded with unreferenced vertices to n_v.  Returns
    vertices (any bit pattern), faces, and the faces that min_faces=2 keeps: the pairs, by construction."""
    periods = n_v // 9 if n_f is None else -(-n_f // 3)
    base = 9 * np.arange(periods, dtype=np.int64)[:, None, None]
    faces = (base + np.array([[0, 1, 2], [1, 3, 2], [5, 6, 7]])).reshape(-1, 3)[:n_f].astype(np.int32)
    i = np.arange(len(faces))
    kept = (i % 3 == 1) | ((i % 3 == 0) & (i + 1 < len(faces)))                 # a pair cut in two is a lone triangle
    n_v = 9 * periods if n_v is None else n_v
    v = np.random.RandomState(n_v % 1000).randint(-2 ** 31, 2 ** 31, (n_v, 3), dtype=np.int64).astype(np.int32).view(np.float32)
    return v, faces, kept


@pytest.mark.parametrize("side", ["vertices", "faces"])
@pytest.mark.parametrize("n", [1024 * 2048, 1024 * 2048 + 1])
def test_compaction_where_the_scan_takes_a_second_block_per_thread(side, n):
    """1024 and 1025 blocks of 2048 vertices, then of faces (the other side then has more): the one-workgroup scan of the block
    counts takes one block per thread, then two.  The expected mesh is a numpy mask and a cumsum."""
    from ngp_pl_amd import mesh
    v, f, kept = pair_soup(n_v=n) if side == "vertices" else pair_soup(n_f=n)
    assert (len(v) if side == "vertices" else len(f)) == n and min(len(v), len(f)) > 300 * 2048
    used = np.zeros(len(v), bool)
    used[f[kept]] = True
    renumber = np.cumsum(used) - 1
    got = mesh.filter_components(to_mesh(v, f), min_faces=2)
    assert got.faces.dtype == torch.int32 and np.array_equal(got.faces.cpu().numpy(), renumber[f[kept]])
    assert np.array_equal(bits(got.vertices), bits(v[used]))


def test_filter_invariants():
    from ngp_pl_amd import mesh
    vol = smooth_volume((64, 64, 64), 11)
    m = mesh.marching_cubes(torch.from_numpy(vol).cuda(), 0.6, ((0, 0, 0), (1, 1, 1)))
    n_v, n_f = m.vertices.shape[0], m.faces.shape[0]
    # colours carry each vertex's index: where a result vertex came from
    m.colors = torch.arange(n_v, device="cuda", dtype=torch.float32)[:, None].repeat(1, 3).contiguous()
    comps = mesh.connected_components(m)
    C = comps.n_components
    assert C >= 3
    fpc = comps.faces_per_component
    for opts in (dict(keep_largest=1), dict(keep_largest=C - 1), dict(min_faces=int(fpc.median())), dict(keep_largest=2, min_faces=int(fpc.min()) + 1)):
        r = mesh.filter_components(m, **opts)
        src = r.colors[:, 0].long()
        assert (src[1:] > src[:-1]).all()                                    # vertices in the input's relative order
        assert torch.equal(r.colors, m.colors[src]) and torch.equal(r.vertices, m.vertices[src]) and torch.equal(r.normals, m.normals[src])
        assert r.faces.min() >= 0 and r.faces.max() < r.vertices.shape[0]
        assert torch.unique(r.faces).numel() == r.vertices.shape[0]          # no unreferenced vertex
        # the faces are the kept input faces, in order: map back and compare with the input's faces of the kept labels
        kept_labels = torch.unique(comps.vertex_label[src])
        fkeep = torch.isin(comps.face_label, kept_labels)
        assert torch.equal(src[r.faces.long()].int(), m.faces[fkeep])
        # selection: conjunction of both rules
        sel = torch.ones(C, dtype=torch.bool, device="cuda")
        if "min_faces" in opts:
            sel &= fpc >= opts["min_faces"]
        if "keep_largest" in opts:
            order = np.lexsort((comps.labels.cpu().numpy(), -fpc.cpu().numpy()))[:opts["keep_largest"]]
            top = torch.zeros_like(sel)
            top[torch.from_numpy(order).cuda()] = True
            sel &= top
        assert torch.equal(kept_labels, comps.labels[sel])
    both = mesh.filter_components(m, keep_largest=2, min_faces=int(fpc.min()) + 1)
    a, b = mesh.filter_components(m, keep_largest=2), mesh.filter_components(m, min_faces=int(fpc.min()) + 1)
    assert both.faces.shape[0] <= min(a.faces.shape[0], b.faces.shape[0])
    # every component kept: the input, bit for bit (every marching-cubes vertex is referenced)
    for opts in (dict(keep_largest=C), dict(keep_largest=C + 5), dict(min_faces=0), dict(min_faces=int(fpc.min()))):
        r = mesh.filter_components(m, **opts)
        assert torch.equal(r.faces, m.faces)
        for x, y in ((r.vertices, m.vertices), (r.normals, m.normals), (r.colors, m.colors)):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert mesh.filter_components(m) is m
    # nothing kept: empty tensors, no error
    for opts in (dict(keep_largest=0), dict(min_faces=n_f + 1), dict(keep_largest=1, min_faces=int(fpc.max()) + 1)):
        e = mesh.filter_components(m, **opts)
        assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3) and e.normals.shape == (0, 3) and e.colors.shape == (0, 3)
        assert e.faces.dtype == torch.int32 and e.vertices.dtype == torch.float32
    with pytest.raises(ValueError):
        mesh.filter_components(m, keep_largest=-1)
    # an empty mesh in, an empty mesh out
    e = mesh.filter_components(mesh.filter_components(m, keep_largest=0), keep_largest=1)
    assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3)
    ec = mesh.connected_components(e)
    assert ec.n_components == 0 and ec.labels.shape == (0,) and ec.vertex_label.shape == (0,)
    # vertices without faces
    lone = mesh.connected_components(mesh.Mesh(m.vertices[:5].contiguous(), m.faces[:0].contiguous()))
    assert lone.n_components == 0 and lone.vertex_label.tolist() == [0, 1, 2, 3, 4]
    none = mesh.filter_components(mesh.Mesh(m.vertices[:5].contiguous(), m.faces[:0].contiguous()), keep_largest=1)
    assert none.vertices.shape == (0, 3) and none.faces.shape == (0, 3)


def test_face_with_an_index_out_of_range_connects_nothing():
    """include/ngp_meshfilter.h: such a face gets label -1, is counted nowhere and is never kept."""
    from ngp_pl_amd import mesh
    f = np.array([[0, 1, 2], [2, 3, 7], [3, 4, 5], [-1, 4, 0], [5, 4, 6]], np.int32)       # V = 7: faces 1 and 3 are out of range
    v = np.arange(21, dtype=np.float32).reshape(7, 3)
    m = to_mesh(v, f)
    c = mesh.connected_components(m)
    assert c.vertex_label.tolist() == [0, 0, 0, 3, 3, 3, 3] and c.face_label.tolist() == [0, -1, 3, -1, 3]
    assert c.labels.tolist() == [0, 3] and c.faces_per_component.tolist() == [1, 2] and c.n_components == 2
    r = mesh.filter_components(m, keep_largest=2)
    assert r.faces.tolist() == [[0, 1, 2], [3, 4, 5], [5, 4, 6]] and torch.equal(r.vertices.cpu(), torch.from_numpy(v))
    r = mesh.filter_components(m, keep_largest=1)
    assert r.faces.tolist() == [[0, 1, 2], [2, 1, 3]] and torch.equal(r.vertices.cpu(), torch.from_numpy(v[3:]))


def test_two_runs_are_bit_identical():
    from ngp_pl_amd import mesh
    v, f, n, c = strip_soup(seed=3, shuffle_faces=True)
    vol = noise_volume(48, 8)
    for m in (to_mesh(v, f, n, c), mesh.marching_cubes(torch.from_numpy(vol).cuda(), 0.7, ((0, 0, 0), (1, 1, 1)))):
        a, b = mesh.connected_components(m), mesh.connected_components(m)
        assert torch.equal(a.vertex_label, b.vertex_label) and torch.equal(a.face_label, b.face_label)
        assert torch.equal(a.labels, b.labels) and torch.equal(a.faces_per_component, b.faces_per_component) and a.n_components == b.n_components
        for opts in (dict(keep_largest=2), dict(min_faces=5)):
            x, y = mesh.filter_components(m, **opts), mesh.filter_components(m, **opts)
            assert torch.equal(x.faces, y.faces) and x.faces.shape[0] > 0
            for p, q in ((x.vertices, y.vertices), (x.normals, y.normals), (x.colors, y.colors)):
                assert (p is None and q is None) or torch.equal(p.view(torch.int32), q.view(torch.int32))


def test_other_device_is_honoured():
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU on this box")
    from ngp_pl_amd import mesh
    vol = torch.from_numpy(smooth_volume((40, 40, 40), 9))
    m1 = mesh.marching_cubes(vol.to("cuda:1"), 0.6, ((0, 0, 0), (1, 1, 1)))
    m0 = mesh.marching_cubes(vol.to("cuda:0"), 0.6, ((0, 0, 0), (1, 1, 1)))
    c1, c0 = mesh.connected_components(m1), mesh.connected_components(m0)
    assert c1.vertex_label.device.index == 1 and torch.equal(c1.vertex_label.cpu(), c0.vertex_label.cpu()) and c1.n_components == c0.n_components
    r1, r0 = mesh.filter_components(m1, keep_largest=1), mesh.filter_components(m0, keep_largest=1)
    assert r1.faces.device.index == 1 and torch.equal(r1.faces.cpu(), r0.faces.cpu()) and torch.equal(r1.vertices.cpu(), r0.vertices.cpu())


def make_model(seed=3):
    """A non-trivial field without training: random hash-grid and MLP parameters."""
    from ngp_pl_amd.networks import NGP
    torch.manual_seed(seed)
    m = NGP(scale=0.5).cuda()
    m.register_training_buffers()
    with torch.no_grad():
        m.xyz_encoder.params.normal_(0, 0.5)
        m.xyz_encoder._half.invalidate()
    return m


def model_threshold(model, res):
    """An iso-level that cuts the random field: the 90th percentile of its density on the lattice."""
    from ngp_pl_amd import mesh
    vol = mesh.density_volume(model, res)
    return float(torch.quantile(vol.view(-1)[:1000000], 0.9).item()), vol


def test_extract_mesh_with_filter_options_and_colors_after_the_filter():
    from ngp_pl_amd import mesh
    model = make_model()
    res = (40, 36, 32)
    thr, vol = model_threshold(model, res)
    # defaults: the parent behaviour, a direct marching_cubes of density_volume
    plain = mesh.extract_mesh(model, res, thr)
    lo, hi = mesh._box(model)
    direct = mesh.marching_cubes(vol, thr, (lo, hi))
    assert plain.faces.shape[0] > 100 and plain.colors is None
    assert torch.equal(plain.faces, direct.faces) and torch.equal(plain.vertices.view(torch.int32), direct.vertices.view(torch.int32))
    assert torch.equal(plain.normals.view(torch.int32), direct.normals.view(torch.int32))
    full = mesh.extract_mesh(model, res, thr, colors=True)
    comps = mesh.connected_components(full)
    assert comps.n_components > 1
    big = int(comps.faces_per_component.max())
    for opts, api in ((dict(keep_largest=1), dict(keep_largest=1)), (dict(min_component_faces=big), dict(min_faces=big)),
                      (dict(keep_largest=3, min_component_faces=9), dict(keep_largest=3, min_faces=9))):
        got = mesh.extract_mesh(model, res, thr, colors=True, **opts)
        want = mesh.filter_components(full, **api)
        assert big <= got.faces.shape[0] <= full.faces.shape[0] and (got.faces.shape[0] < full.faces.shape[0] or "keep_largest" not in opts)
        assert torch.equal(got.faces, want.faces) and torch.equal(got.vertices.view(torch.int32), want.vertices.view(torch.int32))
        assert torch.equal(got.normals.view(torch.int32), want.normals.view(torch.int32))
        assert got.colors.shape == want.colors.shape and torch.allclose(got.colors, want.colors, atol=1e-6)
    nocol = mesh.extract_mesh(model, res, thr, keep_largest=1)
    assert nocol.colors is None and torch.equal(nocol.faces, mesh.filter_components(plain, keep_largest=1).faces)


def read_ply(path):
    """Minimal reader of the binary little-endian PLY save_ply writes: vertex record array, (F, 3) faces."""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    head = blob[:end].decode("ascii").splitlines()
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    n_v = n_f = None
    props = []
    for line in head[2:-1]:
        w = line.split()
        if w[:2] == ["element", "vertex"]:
            n_v = int(w[2])
        elif w[:2] == ["element", "face"]:
            n_f = int(w[2])
        elif w[0] == "property" and n_f is None:
            props.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
    vdt = np.dtype(props)
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    verts = np.frombuffer(blob, vdt, n_v, end)
    faces = np.frombuffer(blob, fdt, n_f, end + vdt.itemsize * n_v)
    assert end + vdt.itemsize * n_v + fdt.itemsize * n_f == len(blob) and (faces["n"] == 3).all()
    return verts, faces["v"]


def test_cli_keep_largest(tmp_path, capsys):
    from ngp_pl_amd import mesh
    model = make_model()
    res = 40
    thr, _ = model_threshold(model, res)
    slim = {"model." + k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt, out = str(tmp_path / "slim.ckpt"), str(tmp_path / "m.ply")
    torch.save(slim, ckpt)
    assert mesh.main(["--ckpt", ckpt, "--scale", "0.5", "--resolution", str(res), "--threshold", repr(thr), "--colors", "--keep-largest", "1",
                      "--out", out]) == 0
    full = mesh.extract_mesh(model, res, thr)
    found = mesh.connected_components(full).n_components
    want = mesh.filter_components(full, keep_largest=1)
    verts, faces = read_ply(out)
    assert found > 1 and 0 < want.faces.shape[0] < full.faces.shape[0]
    assert len(verts) == want.vertices.shape[0] and np.array_equal(faces, want.faces.cpu().numpy())
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), want.vertices.cpu().numpy())
    assert "red" in verts.dtype.names
    # re-labelled, the written mesh is one component
    again = mesh.connected_components(to_mesh(np.stack([verts["x"], verts["y"], verts["z"]], 1), np.ascontiguousarray(faces)))
    assert again.n_components == 1
    last = capsys.readouterr().out.strip().splitlines()[-1]
    assert last == "%s: %d vertices, %d faces, %d components found, 1 kept" % (out, len(verts), len(faces), found)
    # --min-component-faces, and no option: the line and the mesh of before
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--threshold", repr(thr), "--min-component-faces", "12", "--out", out]) == 0
    verts, faces = read_ply(out)
    assert np.array_equal(faces, mesh.filter_components(full, min_faces=12).faces.cpu().numpy())
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--threshold", repr(thr), "--out", out]) == 0
    verts, faces = read_ply(out)
    assert np.array_equal(faces, full.faces.cpu().numpy())
    assert capsys.readouterr().out.strip().splitlines()[-1] == "%s: %d vertices, %d faces" % (out, len(verts), len(faces))
