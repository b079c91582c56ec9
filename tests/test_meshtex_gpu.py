"""GPU: libngp_meshtex.so bit for bit against the numpy restatement (tests/mesh_texture_reference.py): texel points, directions and
UVs as int32 words, validity, face indices and texture bytes exactly, rendered images and depths as int32 words, on the smallest
inputs at which each mechanism can fail (an odd last face, an unfilled last row, atlas sizes across wave and block edges, chunks
that begin mid-row and mid-cell, bad faces, vertices and normals, the clamp, both raster walkers and the box size between them,
ties in depth, culled faces, chunks of cameras), a linear colour field through bake_texture and render_textured, and
extract_mesh(texture=...) and the CLI on a small model.  Nothing here has a tolerance but the derived bound of the linear field."""
import os

import numpy as np
import pytest
import torch

from tests import mesh_texture_reference as TR

pytestmark = pytest.mark.gpu

F = np.float32
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
BOX6 = BOX[0] + BOX[1]


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def to_mesh(v, f, n=None, device="cuda"):
    from ngp_pl_amd import mesh
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return mesh.Mesh(t(np.asarray(v, F)), t(np.asarray(f, np.int32).reshape(-1, 3)), t(None if n is None else np.asarray(n, F)))


def same_words(a, b):
    return (a is None) == (b is None) and (a is None or (a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))))


def random_mesh(n_faces, seed):
    g = np.random.RandomState(seed)
    n_v = n_faces + 2
    v = g.uniform(-0.9, 0.9, (n_v, 3)).astype(F)
    f = np.stack([g.permutation(n_v)[:3] for _ in range(n_faces)]).astype(np.int32)
    n = g.normal(size=(n_v, 3)).astype(F)
    return v, f, n


def check_points(m, tex, v, f, n, T, box=BOX, begin=0, count=None):
    from ngp_pl_amd import mesh
    p, d, ok = mesh.texel_points(m, tex, box, begin, count)
    wp, wd, wok = TR.texel_points(v, f, n, T, box[0] + box[1], begin, count)
    assert p.dtype == torch.float32 and d.dtype == torch.float32 and ok.dtype == torch.uint8 and p.shape == wp.shape and ok.shape == wok.shape
    assert np.array_equal(ok.cpu().numpy(), wok), "%d valid flags differ" % (ok.cpu().numpy() != wok).sum()
    assert np.array_equal(bits(p), bits(wp)), "%d point words differ" % (bits(p) != bits(wp)).sum()
    assert np.array_equal(bits(d), bits(wd)), "%d direction words differ" % (bits(d) != bits(wd)).sum()
    return wp, wd, wok


SIZES = [1, 2, 3, 4, 5, 127, 128, 129]


# ---- 1. texel points: sizes and chunks


@pytest.mark.parametrize("n_faces", SIZES)
def test_texel_points_sizes_and_chunks(n_faces):
    from ngp_pl_amd import mesh
    v, f, n = random_mesh(n_faces, n_faces)
    m = to_mesh(v, f, n)
    for T in (1, 2, 8):
        tex = mesh.texture_atlas(m, T)
        c, W, H = TR.atlas_size(n_faces, T)
        assert (tex.texels, tex.cells_per_row, tex.width, tex.height, tex.image) == (T, c, W, H, None)
        wp, wd, wok = check_points(m, tex, v, f, n, T)
        total = W * H
        # the odd last face's partner and the cells of an unfilled last row are invalid
        assert wok.sum() == n_faces * (T + 4) * (T + 5) // 2 and len(wok) == total >= (n_faces + 1) // 2 * (T + 4) * (T + 5)
        for chunk in (63, 257):
            got = [mesh.texel_points(m, tex, BOX, b, min(chunk, total - b)) for b in range(0, total, chunk)]
            assert np.array_equal(bits(torch.cat([x[0] for x in got])), bits(wp)) and np.array_equal(bits(torch.cat([x[1] for x in got])), bits(wd))
            assert np.array_equal(torch.cat([x[2] for x in got]).cpu().numpy(), wok)
        # chunks of one texel over a window that begins mid-row and mid-cell
        b0 = min(W + T + 2, total - 1)
        n1 = min(150, total - b0)
        got = [mesh.texel_points(m, tex, BOX, b0 + k, 1) for k in range(n1)]
        assert np.array_equal(bits(torch.cat([x[0] for x in got])), bits(wp[b0:b0 + n1])) and np.array_equal(bits(torch.cat([x[1] for x in got])), bits(wd[b0:b0 + n1]))
        assert np.array_equal(torch.cat([x[2] for x in got]).cpu().numpy(), wok[b0:b0 + n1])
        assert mesh.texel_points(m, tex, BOX, total, 0)[0].shape == (0, 3)
        for begin, count in ((-1, 1), (0, total + 1), (total, 1), (5, -1)):
            with pytest.raises(ValueError):
                mesh.texel_points(m, tex, BOX, begin, count)


# ---- 2. texel points: bad input


def test_texel_points_bad_input():
    from ngp_pl_amd import mesh
    nan, inf = F("nan"), F("inf")
    v = F([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0],            # 0-2: a good face
           [nan, 0.1, 0.2], [0.3, 0.3, 0.3],               # 3: a NaN vertex
           [1, 1, 1], [0.6, 1, 1], [1, 0.6, 1],            # 5-7: a face against the box's upper corner: its border leaves the box
           [-1, -1, -1], [-1, -0.5, -1], [-0.5, -1, -1],   # 8-10: and one against the lower corner
           [0.2, 0.2, 0.2], [0, 0, inf]])                  # 11: a degenerate face's only vertex; 12: an infinite vertex
    n = np.tile(F([0, 0, 1]), (len(v), 1))
    n[0] = 0                                               # a zero normal at a corner: the direction is still defined off the corner
    n[5:8] = 0                                             # a face of zero normals: (0, 0, 1)
    n[8] = nan                                             # a NaN normal
    n[11] = [3e38, 3e38, 0]                                # L overflows to inf: the direction is -(n / inf) = -0, which is finite
    n[4] = [inf, 0, 0]
    n_v = len(v)
    f = np.int32([[0, 1, 2], [0, 1, -1], [n_v, 1, 2], [0, 3, 1], [5, 6, 7], [8, 9, 10], [11, 11, 11], [0, 1, 1], [2 ** 31 - 1, 0, 1], [-2 ** 31, 0, 1],
                  [0, 1, 12], [0, 4, 2], [1, 2, 0]])
    m = to_mesh(v, f, n)
    for T in (1, 3, 8):
        tex = mesh.texture_atlas(m, T)
        wp, wd, wok = check_points(m, tex, v, f, n, T)
        owner = TR.owners(len(f), T)[0]
        for bad in (1, 2, 3, 8, 9, 10):                                          # bad indices, the NaN and the infinite vertex
            assert (wok[owner == bad] == 0).all()
        for good in (0, 4, 5, 6, 7, 11, 12):
            assert wok[owner == good].any()
        assert (wp[wok == 0] == F(BOX[0])).all() and (wd[wok == 0] == F([0, 0, 1])).all()
        assert np.isfinite(wp).all() and np.isfinite(wd).all() and (wp >= -1).all() and (wp <= 1).all()
        # the clamp acted: without the box the border texels of the corner faces lie outside it
        free = TR.texel_points(v, f, n, T, (-9, -9, -9, 9, 9, 9))[0]
        assert (free[owner == 4] > 1).any() and (free[owner == 5] < -1).any() and wp[owner == 4].max() == 1 and wp[owner == 5].min() == -1
        assert (wd[owner == 4] == F([0, 0, 1])).all() and (wd[owner == 6] == 0).all() and (wd[owner == 12][:, 2] < 0).any()
        # a launch on a side stream, and a box that is a single point
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            p, d, ok = mesh.texel_points(m, tex, BOX)
        side.synchronize()
        assert np.array_equal(bits(p), bits(wp)) and np.array_equal(bits(d), bits(wd)) and np.array_equal(ok.cpu().numpy(), wok)
        check_points(m, tex, v, f, n, T, box=((0.25, 0.25, 0.0), (0.25, 0.25, 0.0)))
    # no vertices at all: every texel is invalid and nothing is read
    e = to_mesh(np.zeros((0, 3), F), f, np.zeros((0, 3), F))
    p, d, ok = mesh.texel_points(e, mesh.texture_atlas(e, 2), BOX)
    assert not ok.any() and (p == -1).all()
    with pytest.raises(ValueError, match="normals"):
        mesh.texel_points(to_mesh(v, f), mesh.texture_atlas(m, 2), BOX)
    with pytest.raises(ValueError, match="atlas"):
        mesh.texel_points(m, mesh.texture_atlas(to_mesh(v, f[:5]), 2), BOX)
    for box in (((0, 0, 0), (1, 1)), ((0, 0, nan), (1, 1, 1)), ((0, 0, 0), (1, -1, 1)), ((0, 0, 0), (1, 1, inf))):
        with pytest.raises(ValueError, match="box"):
            mesh.texel_points(m, mesh.texture_atlas(m, 2), box)


# ---- 3. face UVs


@pytest.mark.parametrize("n_faces", SIZES)
def test_face_uvs(n_faces):
    from ngp_pl_amd import mesh
    v, f, _ = random_mesh(n_faces, 100 + n_faces)
    f[0] = [-1, 10 ** 6, 0]                                                      # UVs do not look at the indices
    for T in (1, 2, 8, 256):
        tex = mesh.texture_atlas(to_mesh(v, f), T)
        want = TR.face_uvs(n_faces, T)
        assert tex.uvs.dtype == torch.float32 and tex.uvs.shape == (n_faces, 3, 2)
        assert np.array_equal(bits(tex.uvs), bits(want))
        assert (want > 0).all() and (want < 1).all()


# ---- 4 - 6. render


FOCAL, CX, CY = 32.0, 32.5, 16.5
K0 = F([[FOCAL, 0, CX], [0, FOCAL, CY], [0, 0, 1]])
POSE0 = F([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]])        # at the origin, looking along +z: a vertex (x, y, z) lands at (32 x / z + 32.5, ...)
WH0 = (65, 33)


def screen(u, v, z):
    """The world point that POSE0 / K0 project to pixel coordinates (u, v) at depth z."""
    return [(u - CX) / FOCAL * z, (v - CY) / FOCAL * z, z]


def textured(v, f, T, seed=0):
    """A mesh on the GPU with a random texture image, and the image."""
    from ngp_pl_amd import mesh
    m = to_mesh(v, f)
    m.texture = mesh.texture_atlas(m, T)
    image = np.random.RandomState(seed).randint(0, 256, (m.texture.height, m.texture.width, 3)).astype(np.uint8)
    m.texture.image = torch.from_numpy(image).cuda()
    return m, image


def check_render(v, f, T, K=K0, poses=POSE0[None], wh=WH0, near=0.05, background=(0.25, 0.5, 0.75), seed=0, **kw):
    from ngp_pl_amd import mesh
    v, f = np.asarray(v, F), np.asarray(f, np.int32).reshape(-1, 3)
    m, image = textured(v, f, T, seed)
    want = TR.render(v, f, T, image, K, poses, wh, near, background)
    got = mesh.render_textured(m, K, poses, wh, background=background, near=near, return_ids=True, **kw)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[2].shape == want[2].shape
    assert np.array_equal(got[1].cpu().numpy(), want[1]), "%d face indices differ" % (got[1].cpu().numpy() != want[1]).sum()
    assert np.array_equal(bits(got[2]), bits(want[2])), "%d depth words differ" % (bits(got[2]) != bits(want[2])).sum()
    assert np.array_equal(bits(got[0]), bits(want[0])), "%d colour words differ" % (bits(got[0]) != bits(want[0])).sum()
    only = mesh.render_textured(m, K, poses, wh, background=background, near=near, **kw)
    assert same_words(only, got[0])
    return want, m


def box_pixels(v, face, wh=WH0):
    """Pixels of the clipped box of a face under POSE0 / K0, by the rule."""
    u, w, _ = TR.project(np.asarray(v, F), K0, POSE0)
    u, w = u[list(face)], w[list(face)]
    i0, i1 = max(0, int(np.floor(u.min()))), min(wh[0] - 1, int(np.floor(u.max())))
    j0, j1 = max(0, int(np.floor(w.min()))), min(wh[1] - 1, int(np.floor(w.max())))
    return (i1 - i0 + 1) * (j1 - j0 + 1)


def test_render_one_face_over_the_whole_image():
    v = [screen(-200, -100, 2.0), screen(400, -50, 3.0), screen(-100, 300, 1.5)]
    for T in (1, 8):
        (image, ids, depth), _ = check_render(v, [[0, 1, 2]], T)
        assert (ids == 0).all() and np.isfinite(depth).all() and depth.min() > 1.5 and depth.max() < 3.0
        assert len(np.unique(image.reshape(-1, 3), axis=0)) > 500                # the texture varies across the face


def test_render_small_faces_and_the_box_sizes_between_the_walkers():
    g = np.random.RandomState(7)
    v, f = [], []
    for k in range(300):                                                         # boxes of a few pixels: the lane walker
        u0, v0, z = g.uniform(-3, 68), g.uniform(-3, 36), g.uniform(1, 3)
        v += [screen(u0 + g.uniform(-3, 3), v0 + g.uniform(-3, 3), z + g.uniform(-0.2, 0.2)) for _ in range(3)]
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    assert max(box_pixels(v, face) for face in f) <= 64
    (image, ids, depth), _ = check_render(v, f, 2)
    assert 50 < len(np.unique(ids)) and (ids == -1).any() and (ids >= 0).sum() > 100
    # a box of 8 x 8 = 64 pixels is the lane's, one of 13 x 5 = 65 pixels the wave's; alone, together, and under the small faces
    v64 = [screen(10.2, 5.2, 1.0), screen(17.8, 6.0, 1.1), screen(12.0, 12.8, 1.2)]
    v65 = [screen(20.1, 3.3, 1.3), screen(32.9, 5.0, 1.0), screen(25.0, 7.9, 1.1)]
    assert box_pixels(v64, (0, 1, 2)) == 64 and box_pixels(v65, (0, 1, 2)) == 65
    for vv, ff in ((v64, [[0, 1, 2]]), (v65, [[0, 1, 2]]), (v64 + v65, [[0, 1, 2], [3, 4, 5]]), (v65 + v64 + v, [[0, 1, 2], [3, 4, 5]] + [[a + 6 for a in face] for face in f])):
        (_, ids, _), _ = check_render(vv, ff, 3)
        assert (ids == 0).sum() > 10
    # 257 large faces over one another: every wave of a block walks boxes together, and a second block's first lane has one
    big_v, big_f = [], []
    for k in range(257):
        z = g.uniform(1, 3)
        big_v += [screen(g.uniform(-20, 30), g.uniform(-20, 10), z), screen(g.uniform(40, 90), g.uniform(-10, 20), z + 0.1), screen(g.uniform(10, 60), g.uniform(25, 60), z - 0.1)]
        big_f.append([3 * k, 3 * k + 1, 3 * k + 2])
    (_, ids, _), _ = check_render(big_v, big_f, 1)
    assert len(np.unique(ids)) > 5


def test_render_ties():
    tri = [screen(5, 3, 1.0), screen(60, 8, 1.0), screen(20, 30, 1.0)]
    # two coincident faces (the same three vertices, and the same points again): the smaller index wins everywhere
    for v, f in ((tri, [[0, 1, 2], [0, 1, 2]]), (tri + tri, [[3, 4, 5], [0, 1, 2]]), (tri, [[0, 1, 2], [0, 1, 2], [0, 1, 2]])):
        (_, ids, depth), _ = check_render(v, f, 4)
        assert set(np.unique(ids).tolist()) == {-1, 0} and (depth[ids == 0] == 1).all()
    # two abutting faces, the shared edge on the pixel centres of column 20 (u = 20.5 exactly: 32 * -0.375 + 32.5): both cover
    # them at the same depth, the smaller index keeps them
    # every coordinate is a half-integer on the screen, so the edge functions are exact and both faces give z = 1 bit for bit
    a, b, c, d = [-0.375, -0.375, 1.0], [-0.375, 0.3125, 1.0], [-0.75, 0.0, 1.0], [0.25, 0.0, 1.0]
    for f, winner in (([[0, 1, 2], [1, 0, 3]], 0), ([[1, 0, 3], [0, 1, 2]], 0), ([[0, 1, 2], [0, 1, 3]], 0)):
        (_, ids, depth), _ = check_render([a, b, c, d], f, 4)
        column = ids[0, :, 20]
        assert (column == winner).sum() >= 20 and set(column.tolist()) == {-1, winner}
        assert (ids[0, :, 19] == f.index([0, 1, 2])).any() and (ids[0, :, 21] == 1 - f.index([0, 1, 2])).any()


def test_render_culled_and_empty():
    near = 0.5
    v = [screen(5, 5, 1.0), screen(25, 6, 1.0), screen(10, 25, 1.0),                        # 0: seen, counter-clockwise on the screen
         screen(30, 5, 1.0), screen(35, 25, 1.0), screen(50, 6, 1.0),                       # 1: seen, the other winding
         screen(5, 5, 0.4), screen(60, 6, 0.4), screen(10, 30, 0.4),                        # 2: wholly in front of near
         screen(5, 5, 0.8), screen(60, 6, 0.3), screen(10, 30, 0.8),                        # 3: one vertex in front of near: no clipping, dropped
         screen(40, 20, 1.0), screen(50, 25, 1.0), screen(60, 30, 1.0),                     # 4: zero area on the screen (exact coordinates)
         [0.1, 0.1, -1.0], [0.5, 0.1, -1.0], [0.1, 0.5, -1.0]]                              # 5: behind the camera
    f = [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(6)] + [[0, 0, 1], [0, 1, 99], [-1, 1, 2]]
    (image, ids, depth), m = check_render(v, f, 2, near=near)
    assert set(np.unique(ids).tolist()) == {-1, 0, 1}
    empty = ids == -1
    assert empty.sum() > 1000 and (image[empty] == F([0.25, 0.5, 0.75])).all() and np.isposinf(depth[empty]).all()
    # near decides: with a smaller near the face of depth 0.4 is in front of everything it covers
    (_, ids2, _), _ = check_render(v, f, 2, near=0.35)
    assert (ids2 == 2).sum() > 500
    # nothing lands at all: the background alone
    (image3, ids3, _), _ = check_render(v, f, 2, near=10.0, background=(0, 1, 0.5))
    assert (ids3 == -1).all() and (image3 == F([0, 1, 0.5])).all()
    from ngp_pl_amd import mesh
    for bad in dict(background=(1, 1)), dict(background=(1, float("nan"), 1)), dict(near=float("inf")):
        with pytest.raises(ValueError):
            mesh.render_textured(m, K0, POSE0[None], WH0, **bad)
    bare = to_mesh(v, f)
    with pytest.raises(ValueError):
        mesh.render_textured(bare, K0, POSE0[None], WH0)
    bare.texture = mesh.texture_atlas(bare, 2)
    with pytest.raises(ValueError, match="image"):
        mesh.render_textured(bare, K0, POSE0[None], WH0)


@pytest.fixture(scope="module")
def ball():
    """The 24^3 marching-cubes sphere (jittered), its reference texture of the linear colour field at T = 3 and three cameras."""
    v, f, n = TR.sphere_mesh(24, radius=0.7, jitter=0.2, seed=2)
    K, poses, wh = TR.sphere_cameras(3, 48)
    return v, f, n, K, poses, wh


def test_render_cameras_chunks_and_sampling(ball):
    from ngp_pl_amd import mesh
    v, f, n, K, poses, wh = ball
    for T in (1, 3):
        (image, ids, depth), m = check_render(v, f, T, K, poses, wh, near=0.01, seed=T)
        seen = ids[ids >= 0]
        assert (seen & 1).any() and not (seen & 1).all() and len(np.unique(seen)) > 0.3 * len(f)             # both slots sampled
        one = check_render(v, f, T, K, poses[1:2], wh, near=0.01, seed=T)[0]
        assert np.array_equal(bits(one[0][0]), bits(image[1])) and np.array_equal(one[1][0], ids[1])
        # a workspace of one camera: three chunks, the same words; and twice
        a = mesh.render_textured(m, K, poses, wh, background=(0.25, 0.5, 0.75), near=0.01, max_workspace_bytes=8 * wh[0] * wh[1], return_ids=True)
        b = mesh.render_textured(m, K, poses, wh, background=(0.25, 0.5, 0.75), near=0.01, max_workspace_bytes=1, return_ids=True)
        c = mesh.render_textured(m, K, poses, wh, background=(0.25, 0.5, 0.75), near=0.01, max_workspace_bytes=2 * 8 * wh[0] * wh[1], return_ids=True)
        for got in (a, b, c):
            assert np.array_equal(bits(got[0]), bits(image)) and np.array_equal(got[1].cpu().numpy(), ids) and np.array_equal(bits(got[2]), bits(depth))
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            s = mesh.render_textured(m, K, poses, wh, background=(0.25, 0.5, 0.75), near=0.01)
        side.synchronize()
        assert np.array_equal(bits(s), bits(image))


# ---- 7. a linear colour field through bake_texture and render_textured


def torch_linear_colour(p, d):
    g = TR.GRADIENT.astype(F)
    return torch.stack([0.5 + ((float(g[r, 0]) * p[:, 0] + float(g[r, 1]) * p[:, 1]) + float(g[r, 2]) * p[:, 2]) for r in range(3)], 1)


def test_linear_colour_on_the_gpu(ball):
    """The bound of tests/test_meshtex_cpu.py::test_linear_colour_is_reproduced_within_half_a_step, derived there: half a step of
    1 / 255 plus 1e-5 of float rounding."""
    from ngp_pl_amd import mesh
    v, f, n, K, poses, wh = ball
    T = 3
    m = to_mesh(v, f, n)
    want_tex = TR.bake(v, f, n, T, BOX6, TR.linear_colour)
    for chunk in (1 << 20, 1000):
        baked = mesh.bake_texture(None, m, T, chunk=chunk, color_fn=torch_linear_colour, box=BOX)
        assert baked.texture.image.dtype == torch.uint8 and np.array_equal(baked.texture.image.cpu().numpy(), want_tex)
    assert baked.vertices is m.vertices and m.texture is None and np.array_equal(bits(baked.texture.uvs), bits(TR.face_uvs(len(f), T)))
    # without normals the directions come from vertex_normals; the points, and so this texture, are the same
    assert np.array_equal(mesh.bake_texture(None, to_mesh(v, f), T, color_fn=torch_linear_colour, box=BOX).texture.image.cpu().numpy(), want_tex)
    got = mesh.render_textured(baked, K, poses, wh, near=0.01, return_ids=True)
    image, ids, depth, beta, gamma = TR.render(v, f, T, want_tex, K, poses, wh, 0.01, return_weights=True)
    assert np.array_equal(bits(got[0]), bits(image)) and np.array_equal(got[1].cpu().numpy(), ids) and np.array_equal(bits(got[2]), bits(depth))
    covered = ids >= 0
    assert covered.sum() > 0.3 * covered.size and (image[~covered] == 1).all()
    tri = v.astype(np.float64)[f[ids[covered]]]
    bb, gg = beta[covered].astype(np.float64)[:, None], gamma[covered].astype(np.float64)[:, None]
    hit = tri[:, 0] + bb * (tri[:, 1] - tri[:, 0]) + gg * (tri[:, 2] - tri[:, 0])
    err = np.abs(got[0].cpu().numpy()[covered].astype(np.float64) - (0.5 + hit @ TR.GRADIENT.T)).max()
    print("largest colour error %.6f = %.3f steps of 1/255" % (err, err * 255))
    assert err <= 0.5 / 255 + 1e-5
    # colours outside [0, 1] and NaN are clamped; the evaluator's shape is checked
    wild = mesh.bake_texture(None, m, 1, color_fn=lambda p, d: torch.stack([p[:, 0] * 5, p[:, 1] * float("nan"), p[:, 2] * 0 + 0.5], 1), box=BOX)
    img = wild.texture.image.cpu().numpy().reshape(-1, 3)
    ok = TR.texel_points(v, f, n, 1, BOX6)[2] == 1
    assert set(np.unique(img[ok][:, 0]).tolist()) >= {0, 255} and (img[ok][:, 1] == 0).all() and (img[ok][:, 2] == 128).all() and (img[~ok] == 0).all()
    with pytest.raises(ValueError):
        mesh.bake_texture(None, m, 1, color_fn=lambda p, d: p[:, :2], box=BOX)


# ---- 8. end to end on a small model


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


def same_mesh(a, b):
    return torch.equal(a.faces, b.faces) and same_words(a.vertices, b.vertices) and same_words(a.normals, b.normals) and same_words(a.colors, b.colors)


def same_texture(a, b):
    return ((a.texels, a.width, a.height, a.cells_per_row) == (b.texels, b.width, b.height, b.cells_per_row) and same_words(a.uvs, b.uvs)
            and torch.equal(a.image, b.image))


def test_extract_mesh_with_a_texture(true_density):
    from ngp_pl_amd import mesh
    model = make_model()
    res = 48
    plain = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, colors=True)
    none = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, colors=True, texture=None)
    assert same_mesh(plain, none) and plain.texture is None and none.texture is None       # without the option: today's output
    got = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, colors=True, texture=4)
    want = mesh.bake_texture(model, plain, 4)
    assert same_mesh(got, plain) and same_texture(got.texture, want.texture) and got.texture.texels == 4
    assert same_texture(mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, texture=dict(texels=4)).texture, want.texture)
    image = got.texture.image
    assert image.dtype == torch.uint8 and image.shape == (got.texture.height, got.texture.width, 3)
    p, d, ok = mesh.texel_points(plain, want.texture, mesh._box(model))
    assert 0.4 < ok.float().mean() <= 1 and (image.view(-1, 3)[ok == 0] == 0).all() and image.view(-1, 3)[ok == 1].float().std() > 1
    # the texels hold the model's colour at the texel points, seen along minus the normals
    rgb = model(p, d)[1].float()                                                 # one chunk, as bake_texture evaluated it
    assert p.shape[0] <= 1 << 20 and torch.equal(image.view(-1, 3)[ok == 1], torch.round(rgb.clamp(0, 1) * 255).to(torch.uint8)[ok == 1])
    # with smoothing: the geometry of the smoothed mesh, the texture baked before the smoothing
    smooth = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, colors=True, smooth=2, texture=4)
    assert same_mesh(smooth, mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, colors=True, smooth=2))
    assert same_texture(smooth.texture, want.texture) and not same_words(smooth.vertices, plain.vertices)
    # the textured mesh renders; what it shows is the texture's colours
    from ngp_pl_amd import synthetic as syn
    K, poses = syn.intrinsics(64), syn.hemisphere_poses(2, seed=1)
    img, ids, depth = mesh.render_textured(got, K, poses, (64, 64), return_ids=True)
    assert (ids >= 0).float().mean() > 0.05 and torch.isfinite(img).all() and (img[ids < 0] == 1).all() and torch.isinf(depth[ids < 0]).all()


def test_cli_writes_obj_mtl_png(true_density, tmp_path, capsys):
    from ngp_pl_amd import mesh
    from tests.test_meshtex_cpu import read_obj, read_png
    model = make_model()
    res = 48
    slim = {"model." + k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt, out = str(tmp_path / "slim.ckpt"), str(tmp_path / "scene.obj")
    torch.save(slim, ckpt)
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--keep-largest", "1", "--simplify-voxels", "2", "--texture-texels", "3", "--out", out]) == 0
    want = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, texture=3)
    t = want.texture
    last = capsys.readouterr().out.strip().splitlines()[-1]
    assert last.startswith("%s: %d vertices, %d faces, " % (out, want.vertices.shape[0], want.faces.shape[0])) and last.endswith(", texture %d x %d" % (t.width, t.height))
    assert sorted(os.listdir(str(tmp_path))) == ["scene.mtl", "scene.obj", "scene.png", "slim.ckpt"]
    assert np.array_equal(read_png(str(tmp_path / "scene.png")), t.image.cpu().numpy())
    o = read_obj(out)
    n_f = want.faces.shape[0]
    assert np.array_equal(bits(np.asarray(o["v"], np.float64).astype(F)), bits(want.vertices)) and np.array_equal(bits(np.asarray(o["vn"], np.float64).astype(F)), bits(want.normals))
    assert np.array_equal(bits(np.asarray(o["vt"], np.float64).astype(F)), bits(t.uvs.view(-1, 2)))
    faces = np.asarray(o["f"])
    assert faces.shape == (n_f, 3, 3) and np.array_equal(faces[:, :, 0] - 1, want.faces.cpu().numpy()) and np.array_equal(faces[:, :, 1] - 1, np.arange(3 * n_f).reshape(-1, 3))
    assert o["mtllib"] == ["scene.mtl"] and "map_Kd scene.png" in open(str(tmp_path / "scene.mtl")).read()
    # a PLY as before, and its line without a texture
    ply = str(tmp_path / "m.ply")
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--out", ply]) == 0
    full = mesh.extract_mesh(model, res)
    assert capsys.readouterr().out.strip().splitlines()[-1] == "%s: %d vertices, %d faces" % (ply, full.vertices.shape[0], full.faces.shape[0])
