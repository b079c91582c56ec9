"""GPU: the decimation of libngp_meshdecimate.so against the numpy restatement (tests/mesh_decimate_reference.py), bit for bit:
vertices, faces, normals, colours and the totals of every round, on the hand cases, the boxes and the sphere of
tests/test_meshdecimate_cpu.py, on soups at the wave and block edges of the compaction, on fans of MAX_DEGREE and MAX_DEGREE + 1
faces, on bad input between canaries, without attributes, on empty meshes, on a target nothing can reach, twice and on a side
stream, and through extract_mesh(decimate=...) and the CLI.  Nothing here has a tolerance."""
import numpy as np
import pytest
import torch

from tests import mc_reference as R
from tests import mesh_decimate_reference as DR
from tests import test_meshdecimate_cpu as G
from tests import test_meshquadric_cpu as Q
from tests.test_meshsimplify_gpu import bits, make_model, same_mesh, sheet, to_mesh, true_density  # noqa: F401  (true_density is a fixture)

pytestmark = pytest.mark.gpu


def compare(got, stats, want):
    wv, wf, wn, wc, wst = want
    assert got.faces.dtype == torch.int32 and got.faces.shape == wf.shape and np.array_equal(got.faces.cpu().numpy(), wf), "faces differ"
    for name, a, w in (("vertices", got.vertices, wv), ("normals", got.normals, wn), ("colors", got.colors, wc)):
        assert (a is None) == (w is None), name
        if w is not None:
            assert a.dtype == torch.float32 and a.shape == w.shape, name
            assert np.array_equal(bits(a), bits(w)), "%s: %d words differ" % (name, (bits(a) != bits(w)).sum())
    assert stats["totals"].dtype == torch.int64 and np.array_equal(stats["totals"].numpy(), wst["totals"]), (stats["totals"], wst["totals"])
    assert (stats["rounds"], stats["reached"], stats["faces"]) == (wst["rounds"], wst["reached"], wst["faces"])


def check(v, f, cell, target_faces=None, max_error=None, n=None, c=None, want=None):
    """mesh.decimate against the restatement, exactly; returns the restatement's result."""
    from ngp_pl_amd import mesh
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32).reshape(-1, 3)
    if want is None:
        want = DR.decimate(v, f, cell, target_faces, max_error, n, c)
    got, stats = mesh.decimate(to_mesh(v, f, n, c), cell, target_faces=target_faces, max_error=max_error, return_stats=True)
    compare(got, stats, want)
    return want


@pytest.mark.parametrize("n", [4, 5, 6])
def test_hand_cases(n):
    v, f = G.fan(n)
    assert check(v, f, 1.0, max_error=0.0)[4]["totals"].tolist() == [[1, 1, n, 1], [0, 0, n - 2, 0]]
    check(v, f, 1.0, target_faces=n - 1)
    v[0, 2] = 0.25
    check(v, f, 1.0, max_error=0.01)
    check(v, f, 1.0, max_error=0.5)
    v, f = G.fan(n, open_at=1)
    assert check(v, f, 1.0, target_faces=1)[4]["totals"].tolist() == [[0, 0, n - 1, 0]]
    v2, f2 = G.fan(5, z=1.0)
    vb = np.concatenate([G.fan(n)[0], v2[1:]])
    fb = np.concatenate([G.fan(n)[1], np.where(f2 == 0, 0, f2 + n)]).astype(np.int32)
    assert check(vb, fb, 1.0, target_faces=1)[4]["totals"].tolist() == [[0, 0, n + 5, 0]]


def test_a_target_nothing_can_reach():
    from ngp_pl_amd import mesh
    v, f = G.tetrahedron()
    want = check(v, f, 1.0, target_faces=2)
    assert want[4]["totals"].tolist() == [[0, 0, 4, 0]] and not want[4]["reached"]
    got, stats = mesh.decimate(to_mesh(v, f), 1.0, target_faces=2, return_stats=True)
    assert stats["reached"] is False and stats["rounds"] == 0 and got.faces.shape == (4, 3)


@pytest.mark.parametrize("n", [12, 24])
def test_boxes(n):
    v, f = Q.box(n)
    want = check(v, f, 1.0 / n, max_error=0.0, want=G.box_decimated(n))
    assert want[0].shape == (8, 3) and want[1].shape == (12, 3)


@pytest.mark.parametrize("K", [2, 3])
def test_sphere_targets(K):
    v, f = G.sphere()
    g = np.random.RandomState(K)
    want = G.sphere_decimated(K)
    check(v, f, G.SPHERE_CELL, target_faces=len(want[1]), want=want)
    # attributes ride along bit for bit
    n, c = g.randn(*v.shape).astype(np.float32), g.rand(*v.shape).astype(np.float32)
    idx = G.input_index(v, want[0])
    check(v, f, G.SPHERE_CELL, target_faces=len(want[1]), n=n, c=c, want=(want[0], want[1], n[idx], c[idx], want[4]))


@pytest.mark.parametrize("n", [63, 64, 65, 2047, 2048, 2049])
def test_soups_at_wave_and_block_edges(n):
    for n_v, n_f, seed in ((n, n, n), (n, 2 * n - 1, n + 1), (2 * n - 1, n, n + 2)):
        v, f, _ = sheet(n_v, n_f, seed)
        want = check(v, f, 1.0, target_faces=n_f // 2)
        assert want[4]["totals"][0, 2] == n_f
    # a manifold sheet of the same size beside a soup: something collapses across the block edge
    w = 40
    i, j = np.meshgrid(np.arange(w - 1), np.arange(n // (2 * (w - 1)) + 2), indexing="ij")
    a = (j * w + i).reshape(-1)
    grid = np.stack([np.stack([a, a + 1, a + w + 1], 1), np.stack([a, a + w + 1, a + w], 1)], 1).reshape(-1, 3)[:n]
    n_gv = int(grid.max()) + 1
    gv = np.stack([np.arange(n_gv) % w, np.arange(n_gv) // w, np.zeros(n_gv)], 1).astype(np.float32)
    v, f, _ = sheet(n, n, n + 3)
    want = check(np.concatenate([gv, v + np.float32([0, 0, 5])]), np.concatenate([grid, f + n_gv]).astype(np.int32), 1.0, max_error=0.0)
    assert want[4]["rounds"] > 0


@pytest.mark.parametrize("degree", [DR.MAX_DEGREE, DR.MAX_DEGREE + 1])
def test_fans_at_max_degree(degree):
    v, f = G.big_fan(degree)
    key, target, won, totals = DR.evaluate(v, DR.begin(f, len(v)), 1.0, 0.0)
    # the centre collapses at MAX_DEGREE only; the ring's vertices are candidates either way, and judging the centre as their
    # target (it loses to a nearer neighbour) walks its row of `degree` faces
    assert (target[0] >= 0) == (degree == DR.MAX_DEGREE) and (target[1:degree + 1] >= 0).all() and totals[0] == degree + (target[0] >= 0)
    want = check(v, f, 1.0, max_error=0.0)
    assert want[4]["rounds"] > 3
    # off the plane the centre is the cheapest: it goes first, or never
    v[0, 2] = 0.001
    want = check(v, f, 1.0, target_faces=len(f) - 8)
    assert want[4]["reached"]


def _bad_sphere():
    v, f = [a.copy() for a in G.sphere()]
    g = np.random.RandomState(8)
    n_v = len(v)
    rows = g.permutation(n_v)[:120]
    for k, bad in enumerate((np.float32("nan"), np.float32("inf"), -np.float32("inf"), np.float32(3e38))):
        v[rows[30 * k:30 * k + 30], g.randint(0, 3, 30)] = bad
    fr = g.permutation(len(f))[:400]
    for k, bad in enumerate((-1, n_v, 2 ** 31 - 1, -2 ** 31, n_v + 7)):
        f[fr[40 * k:40 * k + 40], g.randint(0, 3, 40)] = bad                   # indices out of range
    f[fr[200:240], 1] = f[fr[200:240], 0]                                      # repeated indices
    f[fr[240:260]] = f[fr[240:260], :1]
    f[fr[260:300]] = f[fr[300:340]]                                            # duplicate faces
    f[fr[340:370]] = f[fr[370:400]][:, [1, 2, 0]]                              # and rotated ones
    return v, f


def test_bad_input_between_canaries():
    """The library driven directly, every buffer between two canary regions: the result equals the restatement's, every call
    returns 0 and no canary changes."""
    from ngp_pl_amd import _meshdecimate_lib as L
    v, f = _bad_sphere()
    g = np.random.RandomState(9)
    n, c = g.randn(*v.shape).astype(np.float32), g.rand(*v.shape).astype(np.float32)
    target = 6000
    wv, wf, wn, wc, wst = DR.decimate(v, f, G.SPHERE_CELL, target, 0.02, n, c)
    assert wst["rounds"] > 5 and len(wf) < len(f) - 300
    n_v, n_f = len(v), len(f)
    PAD = 4096
    held = []

    def guarded(n_bytes, src=None):
        buf = torch.full((PAD + n_bytes + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        if src is not None:
            buf[PAD:PAD + n_bytes] = torch.from_numpy(np.ascontiguousarray(src).view(np.uint8).reshape(-1)).cuda()
        held.append((buf, n_bytes))
        return buf, buf.data_ptr() + PAD

    ws_bytes = L.lib().ngp_meshdecimate_workspace_bytes(n_v, n_f)
    ws_buf = torch.full((256 + PAD + ws_bytes + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = (ws_buf.data_ptr() + PAD + 255) // 256 * 256
    ws_off = ws - ws_buf.data_ptr()
    _, dv = guarded(v.nbytes, v)
    _, df = guarded(f.nbytes, f)
    _, dn = guarded(n.nbytes, n)
    _, dc = guarded(c.nbytes, c)
    tot_buf, dt = guarded(24)
    size_buf, ds = guarded(16)
    s = L.stream()
    assert L.call("ngp_meshdecimate_begin", df, n_v, n_f, ws, ws_bytes, s) == 0
    rows, left = [], None
    while left is None or left > target:
        assert L.call("ngp_meshdecimate_round", dv, n_v, n_f, G.SPHERE_CELL, 0.02, ws, ws_bytes, dt, s) == 0
        n_c, n_w, left = tot_buf[PAD:PAD + 24].view(torch.int64).tolist()
        if left <= target or n_c == 0:
            rows.append([n_c, n_w, left, 0])
            break
        keep = min(n_w, (left - target + 1) // 2)
        assert L.call("ngp_meshdecimate_apply", n_v, n_f, n_w, keep, ws, ws_bytes, s) == 0
        rows.append([n_c, n_w, left, keep])
        left -= 2 * keep
    assert np.array_equal(np.array(rows), wst["totals"])
    assert L.call("ngp_meshdecimate_count", n_v, n_f, ws, ws_bytes, ds, s) == 0
    n_ov, n_of = size_buf[PAD:PAD + 16].view(torch.int64).tolist()
    assert (n_ov, n_of) == (len(wv), len(wf))
    outs = [guarded(12 * n_ov) for _ in range(3)] + [guarded(12 * n_of)]
    assert L.call("ngp_meshdecimate_emit", dv, dn, dc, n_v, n_f, ws, ws_bytes, n_ov, n_of, outs[0][1], outs[1][1], outs[2][1], outs[3][1], s) == 0
    torch.cuda.synchronize()
    for (buf, _), w in zip(outs, (wv, wn, wc, wf)):
        got = buf[PAD:PAD + w.nbytes].cpu().numpy().view(np.int32)
        assert np.array_equal(got, np.ascontiguousarray(w).view(np.int32).reshape(-1))
    for buf, n_bytes in held:
        assert (buf[:PAD] == 0xA5).all() and (buf[PAD + n_bytes:] == 0xA5).all()
    assert (ws_buf[:ws_off] == 0xA5).all() and (ws_buf[ws_off + ws_bytes:] == 0xA5).all()
    # the inputs are as they were
    for (buf, n_bytes), src in zip(held[:4], (v, f, n, c)):
        assert np.array_equal(buf[PAD:PAD + n_bytes].cpu().numpy(), np.ascontiguousarray(src).view(np.uint8).reshape(-1))


@pytest.mark.parametrize("with_normals,with_colors", [(False, False), (True, False), (False, True)])
def test_null_attributes(with_normals, with_colors):
    v, f = G.cap()
    g = np.random.RandomState(2)
    n = g.randn(*v.shape).astype(np.float32) if with_normals else None
    c = g.rand(*v.shape).astype(np.float32) if with_colors else None
    want = check(v, f, G.SPHERE_CELL, target_faces=len(f) // 3, n=n, c=c)
    assert want[4]["reached"] and (want[2] is None) == (n is None) and (want[3] is None) == (c is None)


def test_empty_meshes_and_a_target_above_the_face_count():
    from ngp_pl_amd import mesh
    v, f = G.fan(6)
    z3, zi = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    for m in (to_mesh(z3, zi), to_mesh(v, zi, v, None), to_mesh(z3, f)):
        e, st = mesh.decimate(m, 0.5, max_error=0.0, return_stats=True)
        assert e.vertices.shape == (0, 3) and e.faces.shape == (0, 3) and e.faces.dtype == torch.int32 and st["rounds"] == 0 and st["reached"]
        assert (e.normals is None) == (m.normals is None) and e.colors is None
    m = to_mesh(v, f, v, v)
    for target in (6, 7, 10 ** 9):
        same, st = mesh.decimate(m, 0.5, target_faces=target, return_stats=True)
        assert same is m and st["reached"] and st["rounds"] == 0 and st["faces"] == 6 and st["totals"].shape == (0, 4)
    # every face invalid: all are dropped before the first round
    e, st = mesh.decimate(to_mesh(v, np.full((5, 3), 99, np.int32)), 0.5, target_faces=2, return_stats=True)
    assert e.faces.shape == (0, 3) and e.vertices.shape == (0, 3) and st["totals"].tolist() == [[0, 0, 0, 0]] and st["reached"]


def test_two_runs_and_a_side_stream_are_bit_identical():
    from ngp_pl_amd import mesh
    v, f = G.sphere()
    m = to_mesh(v, f, v, None)
    runs = [mesh.decimate(m, G.SPHERE_CELL, target_faces=5000, return_stats=True) for _ in range(2)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        runs.append(mesh.decimate(m, G.SPHERE_CELL, target_faces=5000, return_stats=True))
    side.synchronize()
    assert runs[0][0].faces.shape[0] == 5000
    for got, st in runs[1:]:
        assert same_mesh(got, runs[0][0]) and torch.equal(st["totals"], runs[0][1]["totals"])


def test_extract_mesh_chain(true_density):  # noqa: F811
    from ngp_pl_amd import mesh
    model = make_model()
    res = 48
    plain = mesh.extract_mesh(model, res, keep_largest=1)
    fp = plain.faces.cpu().numpy()
    assert same_mesh(plain, mesh.extract_mesh(model, res, keep_largest=1, decimate=None))
    lo, hi = mesh._box(model)
    voxel = max((b - a) / (res - 1) for a, b in zip(lo, hi))
    target = plain.faces.shape[0] // 4
    want = mesh.decimate(mesh.Mesh(plain.vertices, plain.faces, plain.normals), voxel, target_faces=target)
    got = mesh.extract_mesh(model, res, keep_largest=1, decimate=target)
    assert same_mesh(got, want) and target - 1 <= got.faces.shape[0] <= target
    fo = got.faces.cpu().numpy()
    assert R.is_closed_oriented(fo) == R.is_closed_oriented(fp) and R.is_closed_oriented(fo)
    assert R.euler(got.vertices.cpu().numpy(), fo) == R.euler(plain.vertices.cpu().numpy(), fp)
    # the options as a dict, max_error in voxels; colours on the surviving vertices, along minus their own normals
    bounded = mesh.extract_mesh(model, res, keep_largest=1, decimate=dict(target_faces=target, max_error=0.25), colors=True)
    wb = mesh.decimate(mesh.Mesh(plain.vertices, plain.faces, plain.normals), voxel, target_faces=target, max_error=0.25 * voxel)
    assert same_mesh(mesh.Mesh(bounded.vertices, bounded.faces, bounded.normals), wb) and bounded.faces.shape[0] >= got.faces.shape[0]
    assert bounded.colors.shape == bounded.vertices.shape
    assert torch.allclose(bounded.colors, mesh.vertex_colors(model, wb.vertices, wb.normals), atol=1e-6)
    # after the clustering
    both = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, decimate=target // 2)
    clustered = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2)
    assert same_mesh(both, mesh.decimate(clustered, voxel, target_faces=target // 2))


def test_cli_flags(true_density, tmp_path, capsys):  # noqa: F811
    from ngp_pl_amd import mesh
    from tests.test_meshfilter_gpu import read_ply
    model = make_model()
    res = 48
    slim = {"model." + k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt, out = str(tmp_path / "slim.ckpt"), str(tmp_path / "m.ply")
    torch.save(slim, ckpt)
    full = mesh.extract_mesh(model, res)
    target = full.faces.shape[0] // 3
    argv = ["--ckpt", ckpt, "--resolution", str(res), "--out", out]
    for extra, opts in ((["--decimate-faces", str(target)], dict(target_faces=target)),
                        (["--decimate-faces", str(target), "--decimate-max-error", "0.5"], dict(target_faces=target, max_error=0.5)),
                        (["--decimate-max-error", "0.125"], dict(max_error=0.125))):
        assert mesh.main(argv + extra) == 0
        want = mesh.extract_mesh(model, res, decimate=opts)
        verts, faces = read_ply(out)
        assert 0 < len(faces) < full.faces.shape[0] and np.array_equal(faces, want.faces.cpu().numpy())
        assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), want.vertices.cpu().numpy())
        last = capsys.readouterr().out.strip().splitlines()[-1]
        assert last == "%s: %d vertices, %d faces, simplified %d -> %d vertices, %d -> %d faces" % (
            out, len(verts), len(faces), full.vertices.shape[0], len(verts), full.faces.shape[0], len(faces))
