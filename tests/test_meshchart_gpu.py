"""GPU: libngp_meshchart.so against the numpy restatement (tests/mesh_chart_reference.py), bit for bit and with no tolerance:
classes, labels, chart ids, rectangles, corner_texels, uvs, texel_face, texel points and directions as int32 words, rendered
images, face indices and depths; sizes at the wave and block edges, the scenes that take all three stages, bad input between
canaries, garbage corner_texels, the derived colour bound on the box, and extract_mesh and the CLI writing .obj and .glb."""
import os

import numpy as np
import pytest
import torch

from tests import mesh_atlas_reference as AR
from tests import mesh_chart_reference as CR
from tests import mesh_texture_reference as TR
from tests.test_meshchart_cpu import charts_of, read_glb, scenes
from tests.test_meshtex_gpu import BOX, BOX6, bits, make_model, same_mesh, same_words, to_mesh, true_density  # noqa: F401

pytestmark = pytest.mark.gpu

F = np.float32
S = 1 / 64


def normals_of(v):
    """Some unit normals: the texel directions only need them to be the same on both sides."""
    n = np.asarray(v, np.float64) + np.asarray([0.01, 0.02, 0.03])
    with np.errstate(all="ignore"):                       # a NaN vertex has a NaN normal
        return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F)


def check_atlas(v, f, s, pad, want=None):
    """chart_atlas of the mesh against the restatement; -> (mesh on the GPU with normals, its ChartTexture, the restatement)."""
    from ngp_pl_amd import mesh
    want = CR.Charts(v, f, s, pad) if want is None else want
    m = to_mesh(v, f, normals_of(v))
    t, dbg = mesh.chart_atlas(m, s, pad, return_debug=True)
    assert (t.width, t.height, t.n_charts, t.pad, t.texel_size) == (want.W, want.H, want.n_charts, pad, float(F(s)))
    assert list(t.charts_per_stage) == want.charts_per_stage + [0] * (3 - len(want.charts_per_stage))
    assert list(t.evicted_per_stage) == want.evicted_per_stage + [0] * (2 - len(want.evicted_per_stage))
    assert np.array_equal(dbg["face_class"].cpu().numpy(), want.face_class)
    assert len(dbg["labels"]) == len(want.labels)
    for got, lab in zip(dbg["labels"], want.labels):
        assert np.array_equal(got.cpu().numpy(), lab)
    assert np.array_equal(t.face_chart.cpu().numpy(), want.face_chart)
    assert np.array_equal(t.chart_rects.cpu().numpy(), want.chart_rects)
    assert t.corner_texels.dtype == torch.int32 and np.array_equal(t.corner_texels.cpu().numpy(), want.corner_texels)
    assert np.array_equal(bits(t.uvs), bits(want.uvs))
    assert t.texel_face.dtype == torch.int32 and np.array_equal(t.texel_face.cpu().numpy(), want.texel_face)
    return m, t, want


def check_points(m, t, v, f, want, chunks=(None,), box=BOX):
    from ngp_pl_amd import mesh
    n = want.W * want.H
    wp, wd, wok = CR.texel_points(v, f, m.normals.cpu().numpy(), want, box[0] + box[1])
    for chunk in chunks:
        if chunk is None:
            ranges = [(0, n)]
        elif chunk == 1:                                  # single texels: a stretch in the middle of the atlas
            ranges = [(b, 1) for b in range(n // 2, min(n, n // 2 + 150))]
        else:
            ranges = [(b, min(chunk, n - b)) for b in range(0, n, chunk)]
        for begin, count in ranges:
            p, d, ok = mesh.texel_points(m, t, box, begin, count)
            assert np.array_equal(bits(p), bits(wp[begin:begin + count])), (chunk, begin)
            assert np.array_equal(bits(d), bits(wd[begin:begin + count])), (chunk, begin)
            assert np.array_equal(ok.cpu().numpy(), wok[begin:begin + count]), (chunk, begin)
    return wp, wd, wok


def painted(m, t, seed):
    g = np.random.RandomState(seed)
    image = g.randint(0, 256, (t.height, t.width, 3)).astype(np.uint8)
    t.image = torch.from_numpy(image).cuda()
    m.texture = t
    return image


def check_render(m, t, v, f, image, cameras=2, size=40, **kw):
    from ngp_pl_amd import mesh
    K, poses, wh = TR.sphere_cameras(cameras, size)
    want = CR.render(v, f, t.corner_texels.cpu().numpy(), image, K, poses, wh, 0.01, (0.25, 0.5, 0.75))
    got = mesh.render_textured(m, K, poses, wh, near=0.01, background=(0.25, 0.5, 0.75), return_ids=True, **kw)
    assert np.array_equal(got[1].cpu().numpy(), want[1]) and np.array_equal(bits(got[2]), bits(want[2]))
    assert np.array_equal(bits(got[0]), bits(want[0])), "%d colour words differ" % (bits(got[0]) != bits(want[0])).sum()
    return want


# ---- 1. sizes at the wave and block edges: bent jittered sheets, so charts of several classes meet


@pytest.mark.parametrize("n_faces", [1, 2, 3, 63, 64, 65, 2047, 2048, 2049])
def test_sheets_of_every_size(n_faces):
    v, f = CR.sheet(n_faces, seed=n_faces)
    for attempt in range(2):                              # everything twice, the second time on a side stream
        stream = torch.cuda.Stream() if attempt else torch.cuda.current_stream()
        with torch.cuda.stream(stream):
            m, t, want = check_atlas(v, f, S, 2)
            check_points(m, t, v, f, want, chunks=(None, 257, 63, 1) if n_faces in (65, 2049) else (None,))
            image = painted(m, t, n_faces)
            # one camera per chunk, and all at once
            check_render(m, t, v, f, image, max_workspace_bytes=8 * 40 * 40)
            if n_faces == 2049:
                check_render(m, t, v, f, image)
        stream.synchronize()
    if n_faces >= 63:
        assert len(set(want.face_class.tolist())) >= 3 and want.charts_per_stage[0] >= 3


# ---- 2. the scenes: all three stages, a non-manifold edge, pad 0, 2 and 8


@pytest.mark.parametrize("name,pad", [("icosphere2", 2), ("icosphere3", 2), ("box", 0), ("box", 2), ("box", 8), ("helicoid", 0), ("helicoid", 2),
                                      ("helicoid", 8), ("book", 2), ("sheet257", 0), ("sheet257", 8)])
def test_scenes(name, pad):
    v, f, s = scenes()[name]
    for attempt in range(2):
        m, t, want = check_atlas(v, f, s, pad, charts_of(name, pad))
        check_points(m, t, v, f, want, chunks=(None, 257))
        check_render(m, t, v, f, painted(m, t, pad))
    if name == "helicoid":
        assert t.charts_per_stage == (1, 1, 48) and t.evicted_per_stage == (96, 48)
    if name == "book":
        assert t.face_chart.tolist() == [0, 0, 1, 0]


# ---- 3. bad input between canaries


def test_bad_input_between_canaries():
    from ngp_pl_amd import _meshchart_lib as L, mesh
    from ngp_pl_amd._lib import ptr, stream
    nan, inf = F("nan"), F("inf")
    v = F([[0, 0, 0], [0.25, 0, 0], [0, 0.25, 0], [0.25, 0.25, 0.05],      # 0-3: two good faces
           [nan, 0.1, 0.2], [4096.0, 0, 0], [0.1, 0.1, inf], [0.00001, 0.00002, 0],   # a NaN, 2^22 sixteenths at s = 1 / 64, an infinity, a sliver
           [-0.3, 0.1, 0.3], [-0.3, 0.3, 0.1], [-0.3, 0.1, 0.1]])           # 8-10: a good face of another class
    n_v = len(v)
    f = np.int32([[0, 1, 2], [1, 3, 2], [0, 1, -1], [n_v, 1, 2], [0, 4, 1], [0, 2, 5], [0, 1, 6], [0, 7, 7], [0, 1, 7], [2 ** 31 - 1, 0, 1],
                  [-2 ** 31, 0, 1], [8, 9, 10], [1, 1, 2]])
    bad = (2, 3, 4, 5, 6, 7, 8, 9, 10, 12)
    for pad in (0, 2):
        m, t, want = check_atlas(v, f, S, pad)
        assert (want.face_class[list(bad)] == 6).all() and (want.face_class[[0, 1, 11]] < 6).all()
        assert (want.face_chart[list(bad)] == -1).all() and not want.corner_texels[list(bad)].any()
        wp, wd, wok = check_points(m, t, v, f, want, chunks=(None, 63))
        assert wok.any() and (wp[wok == 0] == F(BOX[0])).all() and (wd[wok == 0] == F([0, 0, 1])).all() and np.isfinite(wp).all()
        check_render(m, t, v, f, painted(m, t, 1))
    # a mesh without a chart, and one without vertices
    for vv, ff in ((v, f[list(bad)]), (np.zeros((0, 3), F), f)):
        with pytest.raises(ValueError, match="no face of the mesh has a chart"):
            mesh.chart_atlas(to_mesh(vv, ff), S)
    # the raw entry points write nothing outside their outputs
    want = CR.Charts(v, f, S, 2)
    m = to_mesh(v, f, normals_of(v))
    n_f, g = len(f), 64
    dev = "cuda"
    canary = lambda size, dtype, val: torch.full((size + 2 * g,), val, dtype=dtype, device=dev)
    cls, off, vf = canary(n_f, torch.uint8, 0xA5), canary(n_v + 1, torch.int64, -77), canary(3 * n_f, torch.int32, -77)
    lab, chart, cnt = canary(n_f, torch.int32, -77), canary(n_f, torch.int32, -77), canary(2, torch.int64, -77)
    lib = L.lib()
    ws = torch.empty(max(lib.ngp_meshchart_classify_workspace_bytes(n_v, n_f), lib.ngp_meshchart_label_workspace_bytes(n_f)) // 8,
                     dtype=torch.int64, device=dev)
    L.call("ngp_meshchart_classify", ptr(m.vertices), ptr(m.faces), n_v, n_f, S, ptr(cls[g:]), ptr(off[g:]), ptr(vf[g:]), ptr(ws), ws.numel() * 8,
           stream())
    chart[g:g + n_f] = -1
    active = (cls[g:g + n_f] < 6).to(torch.uint8)
    L.call("ngp_meshchart_label", ptr(m.faces), n_v, n_f, ptr(cls[g:]), ptr(active), ptr(off[g:]), ptr(vf[g:]), 1, 0, ptr(lab[g:]), ptr(chart[g:]),
           ptr(cnt[g:]), ptr(ws), ws.numel() * 8, stream())
    n = int(cnt[g].item())
    assert n == want.n_charts == 2
    bnd = canary(4 * n, torch.int32, -77)
    L.call("ngp_meshchart_bounds", ptr(m.vertices), ptr(m.faces), n_v, n_f, S, ptr(chart[g:]), 0, n, ptr(bnd[g:]), stream())
    rects = torch.from_numpy(want.chart_rects.astype(np.int32)).cuda()
    W, H = want.W, want.H
    owner, scratch = canary(W * H, torch.int32, -1), canary(W * H, torch.int32, -1)
    owner[:g], owner[g + W * H:], scratch[:g], scratch[g + W * H:] = 55, 55, 55, 55
    ev = canary(n_f, torch.uint8, 0xA5)
    placed = (ptr(m.vertices), ptr(m.faces), n_v, n_f, S, ptr(chart[g:]), ptr(rects), n, 0, n, 2, W, H, ptr(owner[g:]))
    L.call("ngp_meshchart_raster", *placed, stream())
    L.call("ngp_meshchart_evict", *placed, ptr(ev[g:]), ptr(cnt[g + 1:]), stream())
    assert np.array_equal(owner[g:g + W * H].cpu().numpy().astype(np.int64) & 0xFFFFFFFF, want.owner.reshape(-1))
    L.call("ngp_meshchart_dilate", ptr(owner[g:]), ptr(scratch[g:]), W, H, 2, stream())
    ct, uvs = canary(6 * n_f, torch.int32, -77), canary(6 * n_f, torch.float32, -77.0)
    L.call("ngp_meshchart_corners", ptr(m.vertices), ptr(m.faces), n_v, n_f, S, ptr(chart[g:]), ptr(rects), n, 2, W, H, ptr(ct[g:]), ptr(uvs[g:]),
           stream())
    total = W * H
    pts, dirs, okb = canary(3 * total, torch.float32, -77.0), canary(3 * total, torch.float32, -77.0), canary(total, torch.uint8, 0xA5)
    L.call("ngp_meshchart_texel_points", ptr(m.vertices), ptr(m.faces), ptr(m.normals), n_v, n_f, ptr(ct[g:]), W, H, ptr(owner[g:]), mesh._box6(BOX),
           0, total, ptr(pts[g:]), ptr(dirs[g:]), ptr(okb[g:]), stream())
    for buf, size, val in ((cls, n_f, 0xA5), (off, n_v + 1, -77), (vf, 3 * n_f, -77), (lab, n_f, -77), (chart, n_f, -77), (cnt, 2, -77),
                           (bnd, 4 * n, -77), (owner, total, 55), (scratch, total, 55), (ev, n_f, 0xA5), (ct, 6 * n_f, -77), (uvs, 6 * n_f, -77.0),
                           (pts, 3 * total, -77.0), (dirs, 3 * total, -77.0), (okb, total, 0xA5)):
        assert (buf[:g] == val).all() and (buf[g + size:] == val).all()
    assert np.array_equal(cls[g:g + n_f].cpu().numpy(), want.face_class) and np.array_equal(lab[g:g + n_f].cpu().numpy(), want.labels[0])
    assert np.array_equal(chart[g:g + n_f].cpu().numpy(), want.face_chart) and cnt[g:g + 2].tolist() == [2, 0] and not ev[g:g + n_f].any()
    inr = np.nonzero(((f >= 0) & (f < n_v)).all(1))[0]                       # the table lists the faces with all indices in range
    assert int(off[g + n_v].item()) == 3 * len(inr) and sorted(vf[g:g + 3 * len(inr)].tolist()) == sorted(np.repeat(inr, 3).tolist())
    assert off[g:g + n_v + 1].tolist() == np.concatenate([[0], np.cumsum(np.bincount(f[inr].reshape(-1), minlength=n_v))]).tolist()
    assert (vf[g + 3 * len(inr):g + 3 * n_f] == -1).all()
    uv = CR.plane(want.face_class, want.X)
    for k in range(n):
        pts_k = uv[want.face_chart == k].reshape(-1, 2)
        assert bnd[g + 4 * k:g + 4 * k + 4].tolist() == pts_k.min(0).tolist() + pts_k.max(0).tolist()
    assert np.array_equal(owner[g:g + total].cpu().numpy(), want.texel_face.reshape(-1))
    assert np.array_equal(ct[g:g + 6 * n_f].cpu().numpy().reshape(-1, 3, 2), want.corner_texels) and np.array_equal(bits(uvs[g:g + 6 * n_f]), bits(want.uvs).reshape(-1))
    wp, wd, wok = CR.texel_points(v, f, m.normals.cpu().numpy(), want, BOX6)
    assert np.array_equal(bits(pts[g:g + 3 * total]), bits(wp).reshape(-1)) and np.array_equal(bits(dirs[g:g + 3 * total]), bits(wd).reshape(-1))
    assert np.array_equal(okb[g:g + total].cpu().numpy(), wok)
    # a texture that is not this mesh's is refused
    t = mesh.chart_atlas(m, S)
    for wrong in (dict(width=t.width + 1), dict(height=0), dict(corner_texels=t.corner_texels[:-1]), dict(texel_face=t.texel_face.long()),
                  dict(corner_texels=t.corner_texels.cpu())):
        with pytest.raises((ValueError, RuntimeError)):
            mesh.texel_points(m, mesh.dataclasses.replace(t, **wrong), BOX)
    with pytest.raises(ValueError, match="image"):
        mesh.render_textured(mesh.dataclasses.replace(m, texture=t), *TR.sphere_cameras(1, 16))


# ---- 4. garbage corner_texels


def test_garbage_corner_texels_read_nothing_outside_the_texture():
    """Corners anywhere in int32, the texture between canaries of another value: the outputs are those of the clamp rule, which the
    restatement follows, so a read outside the texture would show as a difference."""
    from ngp_pl_amd import mesh
    v, f, s = scenes()["icosphere2"]
    m, t, want = check_atlas(v, f, s, 2, charts_of("icosphere2"))
    g = np.random.RandomState(9)
    ct = g.randint(-2 ** 31, 2 ** 31, (len(f), 3, 2)).astype(np.int32)
    ct[::5] = g.randint(-64, 16 * t.width + 64, (len(ct[::5]), 3, 2))          # some land in and round the atlas
    ct[1::7] = -1
    ct[2::11] = 2 ** 31 - 1
    image = g.randint(0, 256, (t.height, t.width, 3)).astype(np.uint8)
    guard = 4 * t.width * 3 + 5
    buf = torch.full((image.size + 2 * guard,), 200, dtype=torch.uint8, device="cuda")
    buf[guard:guard + image.size] = torch.from_numpy(image.reshape(-1)).cuda()
    t.image = buf[guard:guard + image.size].view(t.height, t.width, 3)
    t.corner_texels = torch.from_numpy(ct).cuda()
    m.texture = t
    check_render(m, t, v, f, image)
    assert (buf[:guard] == 200).all() and (buf[guard + image.size:] == 200).all()


# ---- 5. the derived bound on the box


def test_box_under_an_affine_colour_within_half_a_step():
    """tests/test_meshchart_cpu.py's test of the same name has the derivation: 0.5 / 255 + 1e-5 on every covered pixel."""
    from ngp_pl_amd import mesh
    v, f, s = scenes()["box"]
    m = to_mesh(v, f, normals_of(v))
    colour = lambda p, d: torch.stack([0.5 + 0.6 * p[:, 0], 0.5 + 0.6 * p[:, 1], 0.5 + 0.6 * p[:, 2]], 1)
    baked = mesh.bake_texture(None, m, texel_size=s, charts=True, color_fn=colour, box=BOX, chunk=1000)
    t = baked.texture
    assert isinstance(t, mesh.ChartTexture) and t.charts_per_stage == (6, 0, 0)
    again = mesh.bake_texture(None, m, texel_size=s, charts=dict(pad=2), color_fn=colour, box=BOX)
    assert torch.equal(again.texture.image, t.image) and same_words(again.texture.uvs, t.uvs)
    K, poses, wh = TR.sphere_cameras(3, 48)
    image, ids, depth = mesh.render_textured(baked, K, poses, wh, near=0.01, return_ids=True)
    _, wid, _, beta, gamma = AR.render(v, f, np.zeros((len(f), 2), np.int32), np.zeros((1, 1, 3), np.uint8), K, poses, wh, 0.01, return_weights=True)
    ids = ids.cpu().numpy()
    assert np.array_equal(ids, wid)
    covered = ids >= 0
    assert covered.sum() > 0.1 * covered.size
    tri = v.astype(np.float64)[f[ids[covered]]]
    bb, gg = beta[covered].astype(np.float64)[:, None], gamma[covered].astype(np.float64)[:, None]
    hit = tri[:, 0] + bb * (tri[:, 1] - tri[:, 0]) + gg * (tri[:, 2] - tri[:, 0])
    err = np.abs(image.cpu().numpy()[covered].astype(np.float64) - CR.affine_colour(hit)).max()
    print("largest colour error %.6f = %.3f steps of 1/255" % (err, err * 255))
    assert err <= 0.5 / 255 + 1e-5


# ---- 6. without charts nothing changes


def test_without_charts_the_outputs_are_those_of_before():
    from ngp_pl_amd import mesh
    v, f, s = scenes()["icosphere2"]
    m = to_mesh(v, f, normals_of(v))
    colour = lambda p, d: (p * 0.7 + 0.5)
    K, poses, wh = TR.sphere_cameras(2, 32)
    for kw in (dict(texels=3), dict(texel_size=0.02, min_texels=2, max_texels=32)):
        a, b = mesh.texture_atlas(m, **kw), mesh.texture_atlas(m, charts=None, **kw)
        assert type(a) is type(b) and not isinstance(a, mesh.ChartTexture) and (a.width, a.height) == (b.width, b.height) and same_words(a.uvs, b.uvs)
        x = mesh.bake_texture(None, m, color_fn=colour, box=BOX, **kw)
        y = mesh.bake_texture(None, m, color_fn=colour, box=BOX, charts=False, **kw)
        assert torch.equal(x.texture.image, y.texture.image) and same_words(x.texture.uvs, y.texture.uvs)
        assert same_words(mesh.render_textured(x, K, poses, wh), mesh.render_textured(y, K, poses, wh))
    # and they are the restatements' still
    want = AR.Atlas(v, f, 0.02, AR.LADDER.index(2), AR.LADDER.index(32))
    assert np.array_equal(bits(a.uvs), bits(want.uvs)) and (a.width, a.height) == (want.W, want.H)


# ---- 7. end to end on a small model


def test_extract_mesh_and_the_cli(true_density, tmp_path, capsys):
    from ngp_pl_amd import mesh
    from tests.test_meshtex_cpu import read_obj, read_png
    model = make_model()
    res = 48
    kw = dict(keep_largest=1, decimate=dict(target_faces=1500))
    plain = mesh.extract_mesh(model, res, **kw)
    got = mesh.extract_mesh(model, res, texture=dict(texel_size=0.75, charts=dict(pad=3)), **kw)
    t = got.texture
    assert same_mesh(got, plain) and isinstance(t, mesh.ChartTexture) and t.pad == 3
    lo, hi = mesh._bounds(model, None)
    size = 0.75 * max((b - a) / (res - 1) for a, b in zip(lo, hi))
    assert t.texel_size == float(F(size))
    direct = mesh.bake_texture(model, plain, texel_size=size, charts=dict(pad=3)).texture
    assert (t.width, t.height, t.n_charts) == (direct.width, direct.height, direct.n_charts) and torch.equal(t.image, direct.image)
    assert same_words(t.uvs, direct.uvs) and torch.equal(t.texel_face, direct.texel_face)
    # the restatement on the extracted mesh
    v, f = plain.vertices.cpu().numpy(), plain.faces.cpu().numpy()
    want = CR.Charts(v, f, size, 3)
    assert (t.width, t.height, t.n_charts) == (want.W, want.H, want.n_charts) and np.array_equal(t.face_chart.cpu().numpy(), want.face_chart)
    assert np.array_equal(t.texel_face.cpu().numpy(), want.texel_face) and np.array_equal(t.corner_texels.cpu().numpy(), want.corner_texels)
    assert t.n_charts < plain.faces.shape[0] // 4
    p, d, ok = mesh.texel_points(plain, t, mesh._box(model))
    rgb = model(p, d)[1].float()
    assert torch.equal(t.image.view(-1, 3)[ok == 1], torch.round(rgb.clamp(0, 1) * 255).to(torch.uint8)[ok == 1]) and (t.image.view(-1, 3)[ok == 0] == 0).all()
    assert torch.equal(ok.view(t.height, t.width) == 1, t.texel_face >= 0)
    # the textured mesh renders and scores
    from ngp_pl_amd import synthetic as syn
    K, poses = syn.intrinsics(64), syn.hemisphere_poses(2, seed=1)
    img, ids, depth = mesh.render_textured(got, K, poses, (64, 64), return_ids=True)
    assert (ids >= 0).float().mean() > 0.05 and torch.isfinite(img).all() and (img[ids < 0] == 1).all()
    record = mesh.compare_renders(model, got, K, poses, (64, 64))
    assert record["cameras"] == 2 and np.isfinite(record["psnr_all"])
    with pytest.raises(ValueError, match="ChartTexture"):
        mesh.bake_normal_map(got, plain, 0.1)
    # the CLI: .obj and .glb
    slim = {"model." + k: x.detach().cpu() for k, x in model.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt, out, glb = str(tmp_path / "slim.ckpt"), str(tmp_path / "scene.obj"), str(tmp_path / "scene.glb")
    torch.save(slim, ckpt)
    common = ["--ckpt", ckpt, "--resolution", str(res), "--keep-largest", "1", "--decimate-faces", "1500", "--texture-texel-size", "0.75",
              "--texture-charts", "--texture-chart-pad", "3"]
    capsys.readouterr()
    assert mesh.main(common + ["--out", out]) == 0
    last = capsys.readouterr().out.strip().splitlines()[-1]
    assert last.startswith("%s: %d vertices, %d faces, " % (out, got.vertices.shape[0], got.faces.shape[0]))
    filled = 100.0 * float((t.texel_face >= 0).float().mean().item())
    assert last.endswith(", texture %d x %d, texel size %.6g, charts per stage %s, evicted faces %s, %.1f%% of the texels filled" % (
        t.width, t.height, t.texel_size, " ".join(str(n) for n in t.charts_per_stage), " ".join(str(n) for n in t.evicted_per_stage), filled))
    assert np.array_equal(read_png(str(tmp_path / "scene.png")), t.image.cpu().numpy())
    o = read_obj(out)
    assert np.array_equal(bits(np.asarray(o["vt"], np.float64).astype(F)), bits(t.uvs.view(-1, 2)))
    assert mesh.main(common + ["--out", glb]) == 0
    assert sorted(os.listdir(str(tmp_path))) == ["scene.glb", "scene.mtl", "scene.obj", "scene.png", "slim.ckpt"]
    doc, binary = read_glb(glb)
    n_split = sum(len(np.unique(f[want.face_chart == k])) for k in range(want.n_charts)) + 3 * int((want.face_chart < 0).sum())
    assert doc["accessors"][1]["count"] <= n_split < 3 * len(f) and doc["accessors"][0]["count"] == 3 * len(f)
    view = doc["bufferViews"][doc["images"][0]["bufferView"]]
    (tmp_path / "inside.png").write_bytes(binary[view["byteOffset"]:view["byteOffset"] + view["byteLength"]])
    assert np.array_equal(read_png(str(tmp_path / "inside.png")), t.image.cpu().numpy())
