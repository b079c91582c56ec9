"""GPU: libngp_meshatlas.so bit for bit against the numpy restatement (tests/mesh_atlas_reference.py): classes, order, counts, face
records and UVs, texel points and directions as int32 words, rendered images and depths as int32 words, at the wave and block
edges of the sort and for class mixes that exercise its stability; bad input between canaries; cross-checks against
libngp_meshtex.so that do not go through the restatement; no bleeding between faces; garbage face records; the scene the feature
is for (a few large faces beside many small ones), where the adaptive atlas must beat the uniform one of the same side; and
extract_mesh and the CLI on a small model.  Nothing here has a tolerance."""
import os

import numpy as np
import pytest
import torch

from tests import mesh_atlas_reference as AR
from tests import mesh_texture_reference as TR
from tests.test_meshtex_gpu import (BOX, BOX6, K0, POSE0, WH0, bits, make_model, same_mesh, same_words, screen, to_mesh,  # noqa: F401
                                    true_density)

pytestmark = pytest.mark.gpu

F = np.float32
S = 2.0 ** -9                                            # texel size of the synthetic meshes: class 15 is an edge of at most 0.5


def classed_mesh(classes, seed):
    """A mesh of len(classes) separate right triangles inside the box whose hypotenuse is 0.9 T_c s long: inside class c, whose
    range ends 0.9 below its upper threshold and at least 0.9 / 0.75 above the lower one.  vertices, faces, normals."""
    g = np.random.RandomState(seed)
    n = len(classes)
    L = 0.9 * np.asarray(AR.LADDER, np.float64)[np.asarray(classes)] * S
    a = g.uniform(-0.5, 0.5, (n, 3))
    b, c = a.copy(), a.copy()
    b[:, 0] += 0.8 * L
    c[:, 1] += 0.6 * L
    perm = np.stack([g.permutation(3) for _ in range(n)])                           # the hypotenuse as ab, bc or ca
    tri = np.stack([a, b, c], 1)[np.arange(n)[:, None], perm]
    v = tri.reshape(-1, 3).astype(F)
    f = np.arange(3 * n, dtype=np.int32).reshape(-1, 3)
    return v, f, g.normal(size=v.shape).astype(F)


def mix(kind, n):
    """The classes of n faces."""
    i = np.arange(n)
    if kind == "one":
        return np.full(n, 3)
    if kind == "alternate":                              # stability: equal classes keep their index order face by face
        return np.where(i % 2 == 0, 2, 4)
    if kind == "ends":                                   # only classes 0 and 15, few of the large ones: the atlas stays small
        return np.where(i % 97 == 0, 15, 0)
    extra = max(n - 16, 0)                               # "all": one face per class, the rest in pairs: 16 odd counts when n is even
    cls = np.concatenate([np.arange(16), np.repeat(np.arange(extra // 2) % 6, 2), np.zeros(extra % 2, np.int64)])[:n]
    return np.random.RandomState(n).permutation(cls)


def classify(m, s=S, cmin=0, cmax=15):
    from ngp_pl_amd import mesh
    return mesh._classify(m.vertices, m.faces, s, cmin, cmax)


def check_atlas(v, f, s=S, lo=1, hi=256, m=None):
    """texture_atlas(texel_size=s) against the restatement: every field.  Returns (mesh, texture, reference atlas)."""
    from ngp_pl_amd import mesh
    m = to_mesh(v, f) if m is None else m
    want = AR.Atlas(v, f, s, AR.LADDER.index(lo), AR.LADDER.index(hi))
    face_class, order, counts = classify(m, s, AR.LADDER.index(lo), AR.LADDER.index(hi))
    assert face_class.dtype == torch.uint8 and order.dtype == torch.int32 and counts.dtype == torch.int64
    assert np.array_equal(face_class.cpu().numpy(), want.face_class), "%d classes differ" % (face_class.cpu().numpy() != want.face_class).sum()
    assert counts.cpu().tolist() == want.counts.tolist()
    assert np.array_equal(order.cpu().numpy(), want.order), "%d ranks differ" % (order.cpu().numpy() != want.order).sum()
    t = mesh.texture_atlas(m, texel_size=s, min_texels=lo, max_texels=hi)
    assert isinstance(t, mesh.AdaptiveTexture) and (t.texel_size, t.min_texels, t.max_texels, t.image) == (float(F(s)), lo, hi, None)
    assert (t.width, t.height, list(t.counts)) == (want.W, want.H, want.counts.tolist())
    assert torch.equal(t.order, order) and np.array_equal(t.face_place.cpu().numpy(), want.face_place)
    assert t.face_texels.dtype == torch.int32 and np.array_equal(t.face_texels.cpu().numpy(), want.face_texels)
    assert t.uvs.dtype == torch.float32 and t.uvs.shape == (len(f), 3, 2) and np.array_equal(bits(t.uvs), bits(want.uvs))
    return m, t, want


def check_points(m, t, v, f, n, want, box=BOX, begin=0, count=None):
    from ngp_pl_amd import mesh
    p, d, ok = mesh.texel_points(m, t, box, begin, count)
    wp, wd, wok = AR.texel_points(v, f, n, want.order, want.counts, box[0] + box[1], begin, count)
    assert p.dtype == torch.float32 and d.dtype == torch.float32 and ok.dtype == torch.uint8 and p.shape == wp.shape and ok.shape == wok.shape
    assert np.array_equal(ok.cpu().numpy(), wok), "%d valid flags differ" % (ok.cpu().numpy() != wok).sum()
    assert np.array_equal(bits(p), bits(wp)), "%d point words differ" % (bits(p) != bits(wp)).sum()
    assert np.array_equal(bits(d), bits(wd)), "%d direction words differ" % (bits(d) != bits(wd)).sum()
    return wp, wd, wok


SIZES = [1, 2, 3, 63, 64, 65, 2047, 2048, 2049, 4097]       # the wave and block edges of the sort


# ---- 1. sizes and class mixes


@pytest.mark.parametrize("kind", ["one", "alternate", "all", "ends"])
@pytest.mark.parametrize("n_faces", SIZES)
def test_sizes_and_class_mixes(n_faces, kind):
    from ngp_pl_amd import mesh
    cls = mix(kind, n_faces)
    v, f, n = classed_mesh(cls, 1000 + n_faces)
    m, t, want = check_atlas(v, f, m=to_mesh(v, f, n))
    assert np.array_equal(want.face_class, cls)                                     # the mesh is what it was built to be
    if kind == "all" and n_faces >= 16 and n_faces % 2 == 0:
        assert (want.counts % 2 == 1).all()
    if kind == "alternate" and n_faces > 1:
        assert np.array_equal(want.order, np.concatenate([np.arange(1, n_faces, 2), np.arange(0, n_faces, 2)]))
    again = classify(m)
    assert torch.equal(again[1], t.order) and again[2].cpu().tolist() == list(t.counts)                   # twice: the same ranks
    total = t.width * t.height
    if total > 1200000:                                  # the texels of the larger atlases are covered by the smaller ones
        return
    wp, wd, wok = check_points(m, t, v, f, n, want)
    assert wok.sum() == ((want.face_texels + 4) * (want.face_texels + 5) // 2).sum()
    b0 = min(t.width + 7, total - 1)                     # chunks of one texel over a window that begins mid-row and mid-cell
    n1 = min(100, total - b0)
    got = [mesh.texel_points(m, t, BOX, b0 + k, 1) for k in range(n1)]
    assert np.array_equal(bits(torch.cat([x[0] for x in got])), bits(wp[b0:b0 + n1])) and np.array_equal(bits(torch.cat([x[1] for x in got])), bits(wd[b0:b0 + n1]))
    assert np.array_equal(torch.cat([x[2] for x in got]).cpu().numpy(), wok[b0:b0 + n1])
    if total <= 60000:
        for chunk in (63, 257):
            got = [mesh.texel_points(m, t, BOX, b, min(chunk, total - b)) for b in range(0, total, chunk)]
            assert np.array_equal(bits(torch.cat([x[0] for x in got])), bits(wp)) and np.array_equal(bits(torch.cat([x[1] for x in got])), bits(wd))
            assert np.array_equal(torch.cat([x[2] for x in got]).cpu().numpy(), wok)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t2 = mesh.texture_atlas(m, texel_size=S)
        p, d, ok = mesh.texel_points(m, t2, BOX)
    side.synchronize()
    assert torch.equal(t2.order, t.order) and torch.equal(t2.face_place, t.face_place) and same_words(t2.uvs, t.uvs)
    assert np.array_equal(bits(p), bits(wp)) and np.array_equal(bits(d), bits(wd)) and np.array_equal(ok.cpu().numpy(), wok)
    assert mesh.texel_points(m, t, BOX, total, 0)[0].shape == (0, 3)
    for begin, count in ((-1, 1), (0, total + 1), (total, 1), (5, -1)):
        with pytest.raises(ValueError):
            mesh.texel_points(m, t, BOX, begin, count)


@pytest.mark.parametrize("kind", ["alternate", "all"])
@pytest.mark.parametrize("n_faces", [64 * 2048, 64 * 2048 + 1])
def test_classify_where_the_scan_takes_a_second_item_per_thread(n_faces, kind):
    """64 and 65 blocks of faces times 16 classes are 1024 and 1040 items of the one-workgroup scan: one per thread and two.  The
    sort alone (no atlas of this size is laid out), the expected values straight from numpy."""
    cls = mix(kind, n_faces)
    v, f, n = classed_mesh(cls, 1000 + n_faces)
    face_class, order, counts = classify(to_mesh(v, f, n))
    assert np.array_equal(face_class.cpu().numpy(), cls)
    assert counts.cpu().tolist() == np.bincount(cls, minlength=16).tolist()
    assert np.array_equal(order.cpu().numpy(), np.argsort(-cls, kind="stable"))


# ---- 2. bad input, between canaries


def test_bad_input_between_canaries():
    from ngp_pl_amd import _meshatlas_lib as A, mesh
    from ngp_pl_amd._lib import ptr, stream
    nan, inf = F("nan"), F("inf")
    v = F([[0, 0, 0], [0.05, 0, 0], [0, 0.05, 0],          # 0-2: a good face
           [nan, 0.1, 0.2], [0.3, 0.3, 0.3],               # 3: a NaN vertex
           [1, 1, 1], [0.9, 1, 1], [1, 0.9, 1],            # 5-7: a face against the box's upper corner: its border leaves the box
           [0.2, 0.2, 0.2], [0, 0, inf], [3e38, 0, 0], [-3e38, 0, 0]])
    n = np.tile(F([0, 0, 1]), (len(v), 1))
    n[5:8] = 0
    n[0] = nan
    n_v = len(v)
    f = np.int32([[0, 1, 2], [0, 1, -1], [n_v, 1, 2], [0, 3, 1], [5, 6, 7], [8, 8, 8], [0, 1, 1], [2 ** 31 - 1, 0, 1], [-2 ** 31, 0, 1], [0, 1, 9],
                  [0, 4, 2], [1, 2, 0], [0, 1, 3], [10, 11, 0]])
    s = 0.01
    for lo, hi in ((1, 256), (2, 6), (4, 4)):
        m, t, want = check_atlas(v, f, s, lo, hi, to_mesh(v, f, n))
        cmin = AR.LADDER.index(lo)
        # bad indices, a NaN, an infinite and an overflowing edge: cmin; the zero-length face too, and it is valid
        for bad in (1, 2, 3, 5, 7, 8, 9, 13):
            assert want.face_class[bad] == cmin
        assert want.face_class[0] == min(max(AR.LADDER.index(8), cmin), AR.LADDER.index(hi))              # 0.0707 / 0.01 -> T = 8
        wp, wd, wok = check_points(m, t, v, f, n, want)
        owner = AR.owners(want.order, want.counts)[0]
        for bad in (1, 2, 3, 7, 8, 9, 12, 13):
            assert (wok[owner == bad] == 0).all()
        for good in (0, 4, 5, 6, 10, 11):
            assert wok[owner == good].any()
        assert wok[owner == 5].all() and (wp[owner == 5] == F(0.2)).all()
        assert (wp[wok == 0] == F(BOX[0])).all() and (wd[wok == 0] == F([0, 0, 1])).all() and np.isfinite(wp).all() and (wp <= 1).all()
        assert wp[owner == 4].max() == 1 and (AR.texel_points(v, f, n, want.order, want.counts, (-9,) * 3 + (9,) * 3)[0][owner == 4] > 1).any()
    # n_vertices = 0: every face has class cmin, every texel is invalid and nothing is read
    e = to_mesh(np.zeros((0, 3), F), f, np.zeros((0, 3), F))
    t = mesh.texture_atlas(e, texel_size=s, min_texels=3)
    assert list(t.counts) == [0, 0, len(f)] + [0] * 13 and torch.equal(t.order.cpu(), torch.arange(len(f), dtype=torch.int32))
    p, d, ok = mesh.texel_points(e, t, BOX)
    assert not ok.any() and (p == -1).all()
    # the raw entry points write nothing outside their outputs
    m = to_mesh(v, f, n)
    n_f, pad = len(f), 64
    want = AR.Atlas(v, f, s)
    cls = torch.full((n_f + 2 * pad,), 0xA5, dtype=torch.uint8, device="cuda")
    order = torch.full((n_f + 2 * pad,), -77, dtype=torch.int32, device="cuda")
    counts = torch.full((16 + 2 * pad,), -77, dtype=torch.int64, device="cuda")
    place = torch.full((2 * n_f + 2 * pad,), -77, dtype=torch.int32, device="cuda")
    uvs = torch.full((6 * n_f + 2 * pad,), -77.0, device="cuda")
    ws = torch.empty(A.lib().ngp_meshatlas_classify_workspace_bytes(n_f) // 8, dtype=torch.int64, device="cuda")
    A.call("ngp_meshatlas_classify", ptr(m.vertices), ptr(m.faces), n_v, n_f, s, 0, 15, ptr(cls[pad:]), ptr(order[pad:]), ptr(counts[pad:]), ptr(ws),
           ws.numel() * 8, stream())
    host = mesh._counts_array(counts[pad:pad + 16].cpu().tolist())
    A.call("ngp_meshatlas_place", ptr(order[pad:]), host, n_f, ptr(place[pad:]), stream())
    A.call("ngp_meshatlas_face_uvs", ptr(place[pad:]), n_f, want.W, want.H, ptr(uvs[pad:]), stream())
    total = want.W * want.H
    pts = torch.full((3 * total + 2 * pad,), -77.0, device="cuda")
    dirs = torch.full((3 * total + 2 * pad,), -77.0, device="cuda")
    okb = torch.full((total + 2 * pad,), 0xA5, dtype=torch.uint8, device="cuda")
    A.call("ngp_meshatlas_texel_points", ptr(m.vertices), ptr(m.faces), ptr(m.normals), n_v, n_f, ptr(order[pad:]), host, mesh._box6(BOX), 0, total,
           ptr(pts[pad:]), ptr(dirs[pad:]), ptr(okb[pad:]), stream())
    for buf, size, canary in ((cls, n_f, 0xA5), (order, n_f, -77), (counts, 16, -77), (place, 2 * n_f, -77), (uvs, 6 * n_f, -77.0), (pts, 3 * total, -77.0),
                              (dirs, 3 * total, -77.0), (okb, total, 0xA5)):
        assert (buf[:pad] == canary).all() and (buf[pad + size:] == canary).all()
    assert np.array_equal(cls[pad:pad + n_f].cpu().numpy(), want.face_class) and np.array_equal(order[pad:pad + n_f].cpu().numpy(), want.order)
    assert np.array_equal(place[pad:pad + 2 * n_f].cpu().numpy().reshape(-1, 2), want.face_place)
    assert np.array_equal(bits(uvs[pad:pad + 6 * n_f]), bits(want.uvs).reshape(-1))
    wp, wd, wok = AR.texel_points(v, f, n, want.order, want.counts, BOX6)
    assert np.array_equal(bits(pts[pad:pad + 3 * total]), bits(wp).reshape(-1)) and np.array_equal(okb[pad:pad + total].cpu().numpy(), wok)
    # a texture that is not this mesh's is refused
    t = mesh.texture_atlas(m, texel_size=s)
    K, poses = np.eye(3, dtype=F), np.zeros((2, 3, 4), F)
    for bad in (dict(counts=(len(f) + 1,) + (0,) * 15), dict(counts=(2,) * 3), dict(counts=None), dict(width=t.width + 1), dict(height=t.height - 1),
                dict(order=t.order[:-1]), dict(face_place=t.face_place.long()), dict(order=t.order.cpu())):
        with pytest.raises((ValueError, RuntimeError)):
            mesh.texel_points(m, mesh.dataclasses.replace(t, **bad), BOX)
    with pytest.raises(ValueError, match="image"):
        mesh.render_textured(mesh.dataclasses.replace(m, texture=t), K0, POSE0[None], WH0)


# ---- 3. cross-checks against libngp_meshtex.so, independent of the restatement's arithmetic


@pytest.mark.parametrize("T", [1, 3, 8, 24])
def test_one_class_is_the_uniform_atlas_texel_for_texel(T):
    """With cmin = cmax the order is the identity, and local texel (i', j') of face f has the point, direction and validity that
    ngp_meshtex_texel_points gives the same (f, i', j') at that T.  The restatements only say which texel is which."""
    from ngp_pl_amd import mesh
    v, f, n = TR.sphere_mesh(8, seed=4)
    f = f.copy()
    f[5, 1] = -1
    v[f[9, 0]] = np.nan
    m = to_mesh(v, f, n)
    ours = mesh.texture_atlas(m, texel_size=0.1, min_texels=T, max_texels=T)
    theirs = mesh.texture_atlas(m, T)
    assert torch.equal(ours.order.cpu(), torch.arange(len(f), dtype=torch.int32)) and list(ours.counts)[AR.LADDER.index(T)] == len(f)
    a = [x.cpu().numpy() for x in mesh.texel_points(m, ours, BOX)]
    b = [x.cpu().numpy() for x in mesh.texel_points(m, theirs, BOX)]
    fa, ia, ja, _ = AR.owners(ours.order.cpu().numpy(), ours.counts)
    fb, ib, jb = TR.owners(len(f), T)
    ka, kb = np.nonzero(fa >= 0)[0], np.nonzero(fb >= 0)[0]
    ka = ka[np.lexsort((ja[ka], ia[ka], fa[ka]))]
    kb = kb[np.lexsort((jb[kb], ib[kb], fb[kb]))]
    assert len(ka) == len(kb) == len(f) * (T + 4) * (T + 5) // 2 and np.array_equal(fa[ka], fb[kb]) and np.array_equal(ia[ka], ib[kb])
    assert np.array_equal(bits(a[0][ka]), bits(b[0][kb])) and np.array_equal(bits(a[1][ka]), bits(b[1][kb])) and np.array_equal(a[2][ka], b[2][kb])
    assert not a[2][fa < 0].any() and 0 < a[2][ka].mean() < 1


@pytest.fixture(scope="module")
def ball():
    """The 16^3 marching-cubes sphere (jittered) at a texel size that gives it at least three classes, three cameras of 64 x 48."""
    from tests.mesh_visibility_reference import intrinsics
    v, f, n = TR.sphere_mesh(16, radius=0.7, jitter=0.25, seed=2)
    _, poses, _ = TR.sphere_cameras(3, 64)
    return v, f, n, intrinsics(64 * 1.2, 32.0, 24.0), poses, (64, 48), 0.03


def painted(m, t, seed):
    image = np.random.RandomState(seed).randint(0, 256, (t.height, t.width, 3)).astype(np.uint8)
    t.image = torch.from_numpy(image).cuda()
    m.texture = t
    return image


def check_render(v, f, s=S, K=K0, poses=POSE0[None], wh=WH0, near=0.05, background=(0.25, 0.5, 0.75), seed=0, lo=1, hi=256, **kw):
    from ngp_pl_amd import mesh
    v, f = np.asarray(v, F), np.asarray(f, np.int32).reshape(-1, 3)
    m = to_mesh(v, f)
    t = mesh.texture_atlas(m, texel_size=s, min_texels=lo, max_texels=hi)
    image = painted(m, t, seed)
    place = t.face_place.cpu().numpy()
    want = AR.render(v, f, place, image, K, poses, wh, near, background)
    got = mesh.render_textured(m, K, poses, wh, background=background, near=near, return_ids=True, **kw)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
    assert np.array_equal(got[1].cpu().numpy(), want[1]), "%d face indices differ" % (got[1].cpu().numpy() != want[1]).sum()
    assert np.array_equal(bits(got[2]), bits(want[2])), "%d depth words differ" % (bits(got[2]) != bits(want[2])).sum()
    assert np.array_equal(bits(got[0]), bits(want[0])), "%d colour words differ" % (bits(got[0]) != bits(want[0])).sum()
    assert same_words(mesh.render_textured(m, K, poses, wh, background=background, near=near, **kw), got[0])
    return want, m


def test_render_against_the_restatement_and_the_uniform_renderer(ball):
    from ngp_pl_amd import mesh
    v, f, n, K, poses, wh, s = ball
    (image, ids, depth), m = check_render(v, f, s, K, poses, wh, near=0.01, seed=3)
    classes = AR.face_classes(v, f, s)
    seen = ids[ids >= 0]
    assert len(np.unique(classes)) >= 3 and len(np.unique(classes[seen])) >= 3 and len(np.unique(seen)) > 0.3 * len(f)
    slots = (m.texture.face_place[:, 1].cpu().numpy() >> 8)[seen]
    assert slots.any() and not slots.all()
    # the face index and the depth are those of the uniform atlas's renderer: the raster does not know the classes
    u = to_mesh(v, f)
    u.texture = mesh.texture_atlas(u, 2)
    u.texture.image = torch.zeros(u.texture.height, u.texture.width, 3, dtype=torch.uint8, device="cuda")
    _, uid, udepth = mesh.render_textured(u, K, poses, wh, background=(0.25, 0.5, 0.75), near=0.01, return_ids=True)
    assert np.array_equal(uid.cpu().numpy(), ids) and np.array_equal(bits(udepth), bits(depth))
    # one camera per chunk, two per chunk, twice, on a side stream: the same words
    bg = (0.25, 0.5, 0.75)
    for ws in (1, 8 * wh[0] * wh[1], 2 * 8 * wh[0] * wh[1]):
        got = mesh.render_textured(m, K, poses, wh, background=bg, near=0.01, max_workspace_bytes=ws, return_ids=True)
        assert np.array_equal(bits(got[0]), bits(image)) and np.array_equal(got[1].cpu().numpy(), ids) and np.array_equal(bits(got[2]), bits(depth))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = mesh.render_textured(m, K, poses, wh, background=bg, near=0.01)
    side.synchronize()
    assert np.array_equal(bits(got), bits(image))


def test_render_ties_culled_and_empty():
    """The scenes of tests/test_meshtex_gpu.py, one camera per chunk, the faces in several classes."""
    s = 0.02
    tri = [screen(5, 3, 1.0), screen(60, 8, 1.0), screen(20, 30, 1.0)]
    for v, f in ((tri, [[0, 1, 2], [0, 1, 2]]), (tri + tri, [[3, 4, 5], [0, 1, 2]]), (tri, [[0, 1, 2], [0, 1, 2], [0, 1, 2]])):
        (_, ids, depth), _ = check_render(v, f, s, max_workspace_bytes=1)
        assert set(np.unique(ids).tolist()) == {-1, 0} and (depth[ids == 0] == 1).all()
    a, b, c, d = [-0.375, -0.375, 1.0], [-0.375, 0.3125, 1.0], [-0.75, 0.0, 1.0], [0.25, 0.0, 1.0]
    for f, winner in (([[0, 1, 2], [1, 0, 3]], 0), ([[1, 0, 3], [0, 1, 2]], 0), ([[0, 1, 2], [0, 1, 3]], 0)):
        (_, ids, depth), _ = check_render([a, b, c, d], f, s, max_workspace_bytes=1)
        column = ids[0, :, 20]
        assert (column == winner).sum() >= 20 and set(column.tolist()) == {-1, winner}
    near = 0.5
    v = [screen(5, 5, 1.0), screen(25, 6, 1.0), screen(10, 25, 1.0), screen(30, 5, 1.0), screen(35, 25, 1.0), screen(50, 6, 1.0),
         screen(5, 5, 0.4), screen(60, 6, 0.4), screen(10, 30, 0.4), screen(5, 5, 0.8), screen(60, 6, 0.3), screen(10, 30, 0.8),
         screen(40, 20, 1.0), screen(50, 25, 1.0), screen(60, 30, 1.0), [0.1, 0.1, -1.0], [0.5, 0.1, -1.0], [0.1, 0.5, -1.0]]
    f = [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(6)] + [[0, 0, 1], [0, 1, 99], [-1, 1, 2]]
    assert len(np.unique(AR.face_classes(F(v), f, s))) >= 3
    poses = np.stack([POSE0, POSE0])
    (image, ids, depth), m = check_render(v, f, s, poses=poses, near=near, max_workspace_bytes=1)
    assert set(np.unique(ids).tolist()) == {-1, 0, 1} and np.array_equal(ids[0], ids[1])
    empty = ids == -1
    assert empty.sum() > 1000 and (image[empty] == F([0.25, 0.5, 0.75])).all() and np.isposinf(depth[empty]).all()
    (_, ids2, _), _ = check_render(v, f, s, near=0.35, max_workspace_bytes=1)
    assert (ids2 == 2).sum() > 500
    (image3, ids3, _), _ = check_render(v, f, s, near=10.0, background=(0, 1, 0.5), max_workspace_bytes=1)
    assert (ids3 == -1).all() and (image3 == F([0, 1, 0.5])).all()
    # no vertices: the background alone
    (_, ids4, _), _ = check_render(np.zeros((0, 3), F), f, s)
    assert (ids4 == -1).all()


def test_cull_tex_and_atlas_depths_agree_bit_for_bit():
    """The three users of the shared rasteriser see one surface: the cull's depth buffer is the depth of the uniform atlas's render and
    of the adaptive atlas's, word for word, and the two renders name the same faces.  A 4 x 4 lattice of small quads (lane walker)
    in front of one face that covers the whole image (wave walker), a medium face between them, a face nearer than near_distance
    and a face of zero area; three cameras of 37 x 29, the renders two cameras to a chunk."""
    from ngp_pl_amd import mesh
    W, H, near, focal = 37, 29, 0.5, 32.0
    K = F([[focal, 0, 18.5], [0, focal, 14.5], [0, 0, 1]])
    at = lambda u, v, z: [(u - 18.5) / focal * z, (v - 14.5) / focal * z, z]            # lands on pixel (u, v) of the first camera
    turn = F([[np.cos(0.05), 0, np.sin(0.05), -0.04], [0, 1, 0, 0.03], [-np.sin(0.05), 0, np.cos(0.05), 0.02]])
    poses = np.stack([POSE0, F([[1, 0, 0, 0.06], [0, 1, 0, -0.05], [0, 0, 1, -0.03]]), turn])
    v, f = [], []
    for j in range(5):
        for i in range(5):
            v.append(at(6.3 + 6.1 * i, 3.2 + 5.7 * j, 1.0 + 0.01 * i - 0.02 * j))
    for j in range(4):
        for i in range(4):
            a = 5 * j + i
            f += [[a, a + 1, a + 6], [a, a + 6, a + 5]]
    small = len(f)
    whole = [at(-80, -40, 2.0), at(150, -40, 2.0), at(18, 160, 2.0)]                    # covers every pixel of every camera
    medium = [at(2, 2, 0.8), at(30, 4, 0.8), at(12, 26, 0.8)]                           # in front of a part of the lattice
    nearer = [at(10, 10, 0.3), at(30, 10, 0.3), at(20, 25, 0.3)]                        # closer than near_distance in every camera
    flat = [at(5, 5, 0.7), at(15, 10, 0.7), at(25, 15, 0.7)]                            # named as (A, A, B): area 0 on every screen
    for tri in (whole, medium, nearer, flat):
        n = len(v)
        f.append([n, n, n + 1] if tri is flat else [n, n + 1, n + 2])
        v += tri
    v, f = F(v), np.asarray(f, np.int32)
    assert len(f) == 36 and small == 32
    # the boxes of the first camera straddle the walkers' threshold of 64 pixels
    uv = v[:, :2] / v[:, 2:] * focal + F([18.5, 14.5])
    lo = np.clip(np.floor(uv[f].min(1)), 0, [W - 1, H - 1])
    hi = np.clip(np.floor(uv[f].max(1)), 0, [W - 1, H - 1])
    area = np.prod(hi - lo + 1, axis=1)
    assert (area[:small] <= 64).all() and area[small] == W * H and area[small + 1] > 64
    views, zb = mesh.vertex_views(to_mesh(v, f), K, poses, (W, H), bias=0.01, near=near, return_zbuffer=True)
    cull = zb.cpu().numpy().view(np.uint32)
    assert cull.shape == (3, H, W)
    u = to_mesh(v, f)
    u.texture = mesh.texture_atlas(u, 2)
    u.texture.image = torch.zeros(u.texture.height, u.texture.width, 3, dtype=torch.uint8, device="cuda")
    a = to_mesh(v, f)
    painted(a, mesh.texture_atlas(a, texel_size=0.02), 5)
    assert len(np.unique(AR.face_classes(v, f, 0.02))) >= 3
    ws = 2 * 8 * W * H                                                                  # two cameras, then one
    _, uid, udepth = mesh.render_textured(u, K, poses, (W, H), near=near, max_workspace_bytes=ws, return_ids=True)
    _, aid, adepth = mesh.render_textured(a, K, poses, (W, H), near=near, max_workspace_bytes=ws, return_ids=True)
    udepth, adepth = udepth.cpu().numpy().view(np.uint32), adepth.cpu().numpy().view(np.uint32)
    assert np.array_equal(cull, udepth), "%d depth words of the cull and the uniform render differ" % (cull != udepth).sum()
    assert np.array_equal(cull, adepth), "%d depth words of the cull and the adaptive render differ" % (cull != adepth).sum()
    uid, aid = uid.cpu().numpy(), aid.cpu().numpy()
    assert np.array_equal(uid, aid)
    # the scene is the one described: every pixel is covered, all three kinds of face win pixels, the culled two never do
    assert (uid >= 0).all() and not np.isin(uid, [small + 2, small + 3]).any()
    for c in range(3):
        assert (uid[c] < small).sum() > 100 and (uid[c] == small).sum() > 100 and (uid[c] == small + 1).sum() > 20


# ---- 4. no bleeding


def test_no_colour_bleeds_from_one_face_into_another(ball):
    """Every texel a face owns, border included, holds the face's colour; every other texel 255.  Colour bytes are 0 or powers of
    two: t * (1 - fx) + t * fx is then exactly t (both products are exact, and fl(1 - fx) + fx rounds to 1 for every fx in [0, 1)),
    likewise over fy, so a pixel whose four texels belong to its face is exactly t / 255, and any weight on a foreign texel shows."""
    from ngp_pl_amd import mesh
    v, f, n, K, poses, wh, s = ball
    m = to_mesh(v, f)
    t = mesh.texture_atlas(m, texel_size=s)
    owner = AR.owners(t.order.cpu().numpy(), t.counts)[0]
    digits = np.array([0, 1, 2, 4, 8, 16, 32, 64, 128], np.uint8)
    k = np.arange(len(f)) * 37 % 729
    colour = np.stack([digits[k % 9], digits[k // 9 % 9], digits[k // 81]], 1)
    image = np.where((owner >= 0)[:, None], colour[np.maximum(owner, 0)], np.uint8(255)).astype(np.uint8).reshape(t.height, t.width, 3)
    t.image = torch.from_numpy(image).cuda()
    m.texture = t
    got, ids, _ = mesh.render_textured(m, K, poses, wh, near=0.01, return_ids=True)
    got, ids = got.cpu().numpy(), ids.cpu().numpy()
    covered = ids >= 0
    assert covered.sum() > 2000 and len(np.unique(ids[covered])) > 300
    want = colour[ids[covered]].astype(F) / F(255)
    assert np.array_equal(bits(got[covered]), bits(want)), "%d pixels are not their face's colour" % (bits(got[covered]) != bits(want)).any(1).sum()


# ---- 5. garbage face records


def test_garbage_face_place_reads_nothing_outside_the_atlas(ball):
    """Records with origins up to 65535 and every bit set in the class word, the texture between canaries of another value: the
    outputs are those of the clamp rule, which the restatement follows, so a read outside the atlas would show as a difference."""
    from ngp_pl_amd import mesh
    v, f, n, K, poses, wh, s = ball
    m = to_mesh(v, f)
    t = mesh.texture_atlas(m, texel_size=s)
    g = np.random.RandomState(9)
    place = g.randint(-2 ** 31, 2 ** 31, (len(f), 2)).astype(np.int32)
    place[::5, 0] &= 0x003F003F                          # some origins land inside the atlas, with a foreign class and slot
    place[1::7] = [-1, -1]
    place[2::11] = [0, 0x7FFFFFFF]
    image = g.randint(0, 256, (t.height, t.width, 3)).astype(np.uint8)
    pad = 4 * t.width * 3 + 5
    buf = torch.full((image.size + 2 * pad,), 200, dtype=torch.uint8, device="cuda")
    buf[pad:pad + image.size] = torch.from_numpy(image.reshape(-1)).cuda()
    t.image = buf[pad:pad + image.size].view(t.height, t.width, 3)
    t.face_place = torch.from_numpy(place).cuda()
    m.texture = t
    want = AR.render(v, f, place, image, K, poses, wh, 0.01)
    got = mesh.render_textured(m, K, poses, wh, near=0.01, return_ids=True)
    assert np.array_equal(got[1].cpu().numpy(), want[1]) and np.array_equal(bits(got[2]), bits(want[2]))
    assert np.array_equal(bits(got[0]), bits(want[0])), "%d colour words differ" % (bits(got[0]) != bits(want[0])).sum()
    assert (buf[:pad] == 200).all() and (buf[pad + image.size:] == 200).all()
    # the UVs of such records follow the masks as well
    uvs = torch.empty(len(f), 3, 2, device="cuda")
    from ngp_pl_amd import _meshatlas_lib as A
    from ngp_pl_amd._lib import ptr, stream
    A.call("ngp_meshatlas_face_uvs", ptr(t.face_place), len(f), t.width, t.height, ptr(uvs), stream())
    assert np.array_equal(bits(uvs), bits(AR.face_uvs(place, t.width, t.height)))


# ---- 6. the point of it


def torch_wave(period):
    def fn(p, d):
        return (0.5 + 0.4 * torch.sin(2.0 * np.pi * p.double() / period)).float()
    return fn


def test_adaptive_atlas_beats_the_uniform_one_of_the_same_side():
    """A box of 12 large faces beside a small sphere of 152 faces (AR.box_and_ball), a colour that is smooth in space, three cameras
    that see both.  Atlas A gives every face T = 4; atlas B is the adaptive one at fit_texel_size to A's larger side.  B has no
    more texels than A, its summed squared error against the colour at every covered pixel's surface point is smaller, and no face
    of B is sampled coarser than its texel size.  The period of the colour is the first of 1.6, 0.8, 0.4 at which the restatement's
    error ratio A / B is at least 2 (it is 185 at 1.6: A's box faces have a texel every 0.3, B's every 0.074).  The bytes of a baked
    texture may differ from the restatement's by one step where sin() differs in the last place between numpy and the device, so
    the errors are the device's own and only the inequality is asserted."""
    from ngp_pl_amd import mesh
    v, f, n = AR.box_and_ball()
    K, poses, wh = TR.sphere_cameras(3, 64)
    T = 4
    _, AW, AH = TR.atlas_size(len(f), T)
    side = max(AW, AH)
    s = AR.fit_texel_size(v, f, side)
    ref = AR.Atlas(v, f, s)
    keys = TR.key_buffers(v, f, K, poses, wh, 0.01)

    def surface(depth, covered):
        ci, jj, ii = np.nonzero(covered)
        Kd, P = K.astype(np.float64), poses.astype(np.float64)[ci]
        ray = np.stack([(ii + 0.5 - Kd[0, 2]) / Kd[0, 0], (jj + 0.5 - Kd[1, 2]) / Kd[1, 1], np.ones(len(ii))], 1) * depth[covered].astype(np.float64)[:, None]
        return np.einsum("nij,nj->ni", P[:, :, :3], ray) + P[:, :, 3]

    def errors(image_a, image_b, depth, covered, period):
        truth = AR.wave_colour(period)(surface(depth, covered)).astype(np.float64)
        return ((image_a[covered] - truth) ** 2).sum(), ((image_b[covered] - truth) ** 2).sum()

    for period in (1.6, 0.8, 0.4):
        fn = AR.wave_colour(period)
        ia, ida, da = TR.render(v, f, T, TR.bake(v, f, n, T, BOX6, fn), K, poses, wh, 0.01, keys=keys)
        ib, _, _ = AR.render(v, f, ref.face_place, AR.bake(v, f, n, ref, BOX6, fn), K, poses, wh, 0.01, keys=keys)
        ea, eb = errors(ia, ib, da, ida >= 0, period)
        if ea >= 2 * eb:
            break
    else:
        raise AssertionError("no period gives the restatement a ratio of 2")
    print("restatement: period %.1f, error A %.4f, B %.4f, ratio %.1f" % (period, ea, eb, ea / eb))
    m = to_mesh(v, f, n)
    A = mesh.bake_texture(None, m, T, color_fn=torch_wave(period), box=BOX)
    assert (A.texture.width, A.texture.height) == (AW, AH)
    size = mesh.fit_texel_size(m, max(A.texture.width, A.texture.height))
    assert size == s
    B = mesh.bake_texture(None, m, texel_size=size, color_fn=torch_wave(period), box=BOX)
    tb = B.texture
    assert isinstance(tb, mesh.AdaptiveTexture) and (tb.width, tb.height, list(tb.counts)) == (ref.W, ref.H, ref.counts.tolist())
    assert max(tb.width, tb.height) <= side and (np.asarray(tb.counts) > 0).sum() >= 2
    ga, gida, gda = [x.cpu().numpy() for x in mesh.render_textured(A, K, poses, wh, near=0.01, return_ids=True)]
    gb, gidb, gdb = [x.cpu().numpy() for x in mesh.render_textured(B, K, poses, wh, near=0.01, return_ids=True)]
    covered = gida >= 0
    assert np.array_equal(gida, gidb) and np.array_equal(bits(gda), bits(gdb)) and (gida[covered] < 12).sum() > 3000 and (gida[covered] >= 12).sum() > 100
    ea, eb = errors(ga, gb, gda, covered, period)
    texels_a, texels_b = A.texture.width * A.texture.height, tb.width * tb.height
    spacing = AR.face_spacing(v, f, tb.face_texels.cpu().numpy())
    print("device: texels A %d, B %d; error A %.4f, B %.4f, ratio %.1f; largest spacing %.6f at texel size %.6f"
          % (texels_a, texels_b, ea, eb, ea / eb, spacing.max(), size))
    assert texels_b <= texels_a
    assert eb < ea
    # the class rule compares f32 squares: m <= t * t holds up to three roundings of 2^-24, 1e-6 of the length
    assert spacing.max() <= size * (1 + 1e-6)
    assert mesh.compare_renders.__doc__ and mesh.render_textured(B, K, poses, wh, near=0.01).shape == (3, 64, 64, 3)


# ---- 7. end to end on a small model


def test_extract_mesh_and_the_cli(true_density, tmp_path, capsys):
    from ngp_pl_amd import mesh
    from tests.test_meshtex_cpu import read_obj, read_png
    model = make_model()
    res = 48
    kw = dict(keep_largest=1, decimate=dict(target_faces=1500))
    plain = mesh.extract_mesh(model, res, **kw)
    assert plain.texture is None and plain.faces.shape[0] <= 1500
    # texture=T gives the bits of before: bake_texture's on the same mesh, a Texture
    uniform = mesh.extract_mesh(model, res, texture=3, **kw)
    want = mesh.bake_texture(model, plain, 3).texture
    assert same_mesh(uniform, plain) and isinstance(uniform.texture, mesh.Texture) and uniform.texture.texels == 3
    assert (uniform.texture.width, uniform.texture.height) == (want.width, want.height) and same_words(uniform.texture.uvs, want.uvs)
    assert torch.equal(uniform.texture.image, want.image)
    # texel_size in voxels of the lattice
    got = mesh.extract_mesh(model, res, texture=dict(texel_size=0.75, min_texels=2, max_texels=64), **kw)
    t = got.texture
    assert same_mesh(got, plain) and isinstance(t, mesh.AdaptiveTexture) and (t.min_texels, t.max_texels) == (2, 64)
    lo, hi = mesh._bounds(model, None)
    size = 0.75 * max((b - a) / (res - 1) for a, b in zip(lo, hi))
    assert t.texel_size == float(F(size))
    direct = mesh.bake_texture(model, plain, texel_size=size, min_texels=2, max_texels=64).texture
    assert (t.width, t.height, t.counts) == (direct.width, direct.height, direct.counts) and torch.equal(t.image, direct.image) and same_words(t.uvs, direct.uvs)
    assert sum(t.counts) == plain.faces.shape[0] and sum(c > 0 for c in t.counts) >= 3 and not any(t.counts[:1]) and not any(t.counts[12:])
    p, d, ok = mesh.texel_points(plain, t, mesh._box(model))
    rgb = model(p, d)[1].float()
    assert torch.equal(t.image.view(-1, 3)[ok == 1], torch.round(rgb.clamp(0, 1) * 255).to(torch.uint8)[ok == 1]) and (t.image.view(-1, 3)[ok == 0] == 0).all()
    # max_side goes through fit_texel_size
    fitted = mesh.extract_mesh(model, res, texture=dict(max_side=256), **kw).texture
    assert fitted.texel_size == mesh.fit_texel_size(plain, 256) and max(fitted.width, fitted.height) <= 256
    # the textured mesh renders and scores
    from ngp_pl_amd import synthetic as syn
    K, poses = syn.intrinsics(64), syn.hemisphere_poses(2, seed=1)
    img, ids, depth = mesh.render_textured(got, K, poses, (64, 64), return_ids=True)
    assert (ids >= 0).float().mean() > 0.05 and torch.isfinite(img).all() and (img[ids < 0] == 1).all()
    record = mesh.compare_renders(model, got, K, poses, (64, 64))
    assert record["cameras"] == 2 and np.isfinite(record["psnr_all"])
    # the CLI
    slim = {"model." + k: x.detach().cpu() for k, x in model.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt, out = str(tmp_path / "slim.ckpt"), str(tmp_path / "scene.obj")
    torch.save(slim, ckpt)
    capsys.readouterr()
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--keep-largest", "1", "--decimate-faces", "1500", "--texture-texel-size", "0.75",
                      "--texture-min-texels", "2", "--texture-max-texels", "64", "--out", out]) == 0
    last = capsys.readouterr().out.strip().splitlines()[-1]
    assert last.startswith("%s: %d vertices, %d faces, " % (out, got.vertices.shape[0], got.faces.shape[0]))
    assert (", texture %d x %d, texel size %.6g, faces per texels " % (t.width, t.height, t.texel_size)) in last
    assert last.endswith(" ".join("%d:%d" % (T, c) for T, c in zip(AR.LADDER, t.counts) if c))
    assert sorted(os.listdir(str(tmp_path))) == ["scene.mtl", "scene.obj", "scene.png", "slim.ckpt"]
    assert np.array_equal(read_png(str(tmp_path / "scene.png")), t.image.cpu().numpy())
    o = read_obj(out)
    assert np.array_equal(bits(np.asarray(o["vt"], np.float64).astype(F)), bits(t.uvs.view(-1, 2)))
    assert np.array_equal(bits(np.asarray(o["v"], np.float64).astype(F)), bits(got.vertices))
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--keep-largest", "1", "--decimate-faces", "1500", "--texture-max-side", "256", "--out", out]) == 0
    assert (", texture %d x %d, " % (fitted.width, fitted.height)) in capsys.readouterr().out.strip().splitlines()[-1]
