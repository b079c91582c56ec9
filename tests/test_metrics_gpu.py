"""GPU: libngp_metrics.so against the numpy restatement (tests/metrics_reference.py).  SSIM maps bit for bit as int32 words at
image sizes on and around the kernel's tile edges, for 1, 3 and 4 channels, both layouts and batches; counts exactly; f64 sums
within the bound that holds for any order of additions, and the same 64 bits twice; identical images exactly 1; masks; the
squared error at element counts around the wave, the workgroup and the grid stride; refused calls leave their outputs alone; the
two metric classes, evaluate_frames, mesh.compare_renders and the CLI's --score-cameras against the restatement applied to what
they return."""
import json
import math

import numpy as np
import pytest
import torch

from tests import metrics_reference as R

pytestmark = pytest.mark.gpu

F = np.float32
ONE = 0x3F800000


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def words(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32)


def gpu_ssim(p, t, dr, mask=None, layout="hwc", want_map=True):
    """sum (n,) f64, count (n,) i64 and the map as numpy arrays, straight from ngp_metrics_ssim."""
    from ngp_pl_amd import metrics
    pd, td, md, (n, c, h, w), _ = metrics._images(dev(p), dev(t), None if mask is None else dev(mask), layout, 11)
    total, count, smap = metrics._ssim(pd, td, md, n, c, h, w, layout, float(dr), want_map)
    return total.cpu().numpy(), count.cpu().numpy(), None if smap is None else smap.cpu().numpy()


def sum_bound(count, largest):
    """|any order of f64 additions - the exact sum| of `count` terms of magnitude <= largest: every partial sum is at most
    count * largest and each of the count - 1 additions rounds once."""
    return count * 2.0 ** -53 * largest * count


def check_sums(got_sum, got_count, want_sums, want_counts, largest=1.0):
    assert got_count.tolist() == want_counts
    for s, k, want in zip(got_sum.tolist(), want_counts, want_sums):
        assert abs(s - want) <= sum_bound(k, largest), (s, want, k)
        if k:
            assert sum_bound(k, largest) / k < 1e-9 and abs(s / k - want / k) < 1e-9


@pytest.fixture(scope="module")
def runs():
    """Every case of metrics_reference.cases at the library's tile: the restatement once, the library twice."""
    from ngp_pl_amd import _metrics_lib as L
    out = []
    for case in R.cases(L.TILE_W, L.TILE_H):
        p, t, dr = R.case_images(case)
        want = R.ssim_f32(p, t, dr, None, case[5])
        out.append((case, want, gpu_ssim(p, t, dr, None, case[5]), gpu_ssim(p, t, dr, None, case[5], want_map=False)))
    return out


# ---- 1. maps, counts and sums


def test_maps_bit_for_bit(runs):
    for case, (want_map, _, _), (_, _, got_map), _ in runs:
        assert got_map.shape == want_map.shape and got_map.dtype == np.float32, case
        same = words(got_map) == words(want_map)
        assert same.all(), (case, int((~same).sum()), np.argwhere(~same)[:4].tolist())


def test_counts_exact_and_sums_within_the_f64_bound(runs):
    for case, (want_map, want_sums, want_counts), (got_sum, got_count, _), _ in runs:
        kind, n, h, w, c, layout = case
        assert want_counts == [(h - 10) * (w - 10) * c] * n
        largest = float(np.abs(want_map).max())
        assert largest <= 1.0 + 1e-6
        check_sums(got_sum, got_count, want_sums, want_counts, max(largest, 1.0))


def test_two_runs_give_the_same_64_bits_with_and_without_the_map(runs):
    for case, _, (s1, k1, _), (s2, k2, _) in runs:
        assert s1.view(np.int64).tolist() == s2.view(np.int64).tolist() and k1.tolist() == k2.tolist(), case


def test_identical_images_score_exactly_one():
    from ngp_pl_amd import metrics
    for kind, layout in (("noise", "hwc"), ("quantised", "chw"), ("range4", "hwc"), ("white", "chw")):
        p, _, dr = R.images(kind, 2, 35, 139, 3)
        if layout == "chw":
            p = np.ascontiguousarray(np.moveaxis(p, -1, 1))
        total, count, smap = gpu_ssim(p, p.copy(), dr, None, layout)
        assert (words(smap) == ONE).all()
        assert count.tolist() == [25 * 129 * 3] * 2 and total.tolist() == [float(25 * 129 * 3)] * 2          # ones add exactly in f64
        score = metrics.ssim(dev(p), dev(p.copy()), dr, layout=layout)
        assert score.dtype == torch.float64 and score.tolist() == [1.0, 1.0]
    one = metrics.ssim(dev(p[0]), dev(p[0].copy()), dr, layout=layout, return_map=True)                      # a single image, no leading n
    assert one[0].tolist() == [1.0] and one[1].shape == (3, 25, 129)


def test_images_past_2_to_the_31_elements_score_as_they_do_alone():
    """Ten images of 7800 x 7800 x 4: the last one lies wholly past element 2^31 of the batch.  An image's sum is a function of
    the image and the launch geometry of one image alone, so the batch's entries equal, bit for bit, those of the image scored
    on its own, which a 32-bit index anywhere in the addressing would not give; the images differ, so a wrong offset shows."""
    from ngp_pl_amd import metrics
    n, side, c = 10, 7800, 4
    assert (n - 1) * side * side * c > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(11)
    p = torch.rand(n * side * side * c, device="cuda", generator=g)
    t = torch.rand(n * side * side * c, device="cuda", generator=g)
    for layout, shape in (("hwc", (n, side, side, c)), ("chw", (n, c, side, side))):
        pv, tv = p.view(shape), t.view(shape)
        total, count, _ = metrics._ssim(pv, tv, None, n, c, side, side, layout, 1.0, False)
        se, k = metrics.sq_error(pv, tv, layout=layout)
        for i in (0, n - 1):
            one_total, one_count, _ = metrics._ssim(pv[i:i + 1], tv[i:i + 1], None, 1, c, side, side, layout, 1.0, False)
            one_se, one_k = metrics.sq_error(pv[i:i + 1], tv[i:i + 1], layout=layout)
            assert torch.equal(total[i:i + 1].view(torch.int64), one_total.view(torch.int64)) and torch.equal(count[i:i + 1], one_count)
            assert torch.equal(se[i:i + 1].view(torch.int64), one_se.view(torch.int64)) and torch.equal(k[i:i + 1], one_k)
        assert count.tolist() == [(side - 10) ** 2 * c] * n and k.tolist() == [side * side * c] * n
        assert len(set(total.tolist())) == n and len(set(se.tolist())) == n                         # ten different images
        assert all(abs(x / (side * side * c) - 1 / 6) < 1e-3 for x in se.tolist())                  # E (u - v)^2 = 1/6 for uniform noise


# ---- 2. masks


def test_masks():
    from ngp_pl_amd import metrics
    n, h, w, c = 2, 23, 75, 3
    p, t, dr = R.images("smooth", n, h, w, c)
    want_map, _, _ = R.ssim_f32(p, t, dr)
    g = np.random.RandomState(5)
    random = (g.rand(n, h, w) < 0.4).astype(np.uint8) * g.randint(1, 256, (n, h, w)).astype(np.uint8)       # any non-zero byte selects
    border = np.ones((n, h, w), np.uint8)
    border[:, 5:h - 5, 5:w - 5] = 0                                                                        # true only within 5 pixels of the border
    single = np.zeros((n, h, w), np.uint8)
    single[1, 5 + 12, 5 + 64] = 1                                                                          # window (12, 64): the last tile's corner
    for mask in (random, border, single):
        _, want_sums, want_counts = R.ssim_f32(p, t, dr, mask)
        for want_the_map in (False, True):
            total, count, smap = gpu_ssim(p, t, dr, mask, "hwc", want_the_map)
            check_sums(total, count, want_sums, want_counts)
            if want_the_map:
                assert (words(smap) == words(want_map)).all()                                              # masked-out entries are written all the same
    _, sums, counts = R.ssim_f32(p, t, dr, single)
    assert counts == [0, c] and sums[1] == math.fsum(float(x) for x in want_map[1, 12, 64])
    total, count, _ = gpu_ssim(p, t, dr, border, "hwc", False)
    assert count.tolist() == [0, 0] and total.tolist() == [0.0, 0.0]
    score = metrics.ssim(dev(p), dev(t), dr, mask=dev(border))
    assert torch.isnan(score).all() and torch.isnan(metrics.psnr(dev(p), dev(t), dr, mask=torch.zeros(n, h, w, dtype=torch.bool, device="cuda"))).all()
    # planar, a bool mask through the Python surface
    pc, tc = np.ascontiguousarray(np.moveaxis(p, -1, 1)), np.ascontiguousarray(np.moveaxis(t, -1, 1))
    _, want_sums, want_counts = R.ssim_f32(pc, tc, dr, random, "chw")
    score = metrics.ssim(dev(pc), dev(tc), dr, mask=dev(random != 0), layout="chw").tolist()
    assert all(abs(s - a / b) < 1e-9 for s, a, b in zip(score, want_sums, want_counts))


# ---- 3. the squared error


def gpu_sq(p, t, mask, layout):
    from ngp_pl_amd import metrics
    total, count = metrics.sq_error(dev(p), dev(t), None if mask is None else dev(mask), layout)
    return total.cpu().numpy(), count.cpu().numpy()


def test_squared_error_at_the_wave_workgroup_and_grid_stride_edges():
    from ngp_pl_amd import _metrics_lib as L
    stride = L.SQ_MAX_BLOCKS * L.SQ_THREADS
    # stride + 1 = 3 * 43691 and stride + 2 = 2 * 65537 have no h x w within the side limit; stride + 3 = 25 * 5243 is the first
    # size above the stride that has: three threads take a second trip
    shapes = [(1, e) for e in (1, 63, 64, 65, 255, 256, 257)] + [(25, (stride + 3) // 25)]
    assert 25 * ((stride + 3) // 25) == stride + 3
    g = np.random.RandomState(9)
    for h, w in shapes:
        for c, layout in ((1, "hwc"), (3, "hwc"), (3, "chw"), (4, "chw")) if h == 1 else ((1, "hwc"),):
            shape = (2, h, w, c) if layout == "hwc" else (2, c, h, w)
            p, t = g.rand(*shape).astype(F), g.rand(*shape).astype(F)
            mask = (g.rand(2, h, w) < 0.5).astype(np.uint8)
            for m in (None, mask):
                want_sums, want_counts = R.sq_error_f32(p, t, m, layout)
                a, b = gpu_sq(p, t, m, layout), gpu_sq(p, t, m, layout)
                check_sums(a[0], a[1], want_sums, want_counts)                                             # |d * d| <= 1
                assert a[0].view(np.int64).tolist() == b[0].view(np.int64).tolist() and a[1].tolist() == b[1].tolist()
                if m is None:
                    assert want_counts == [h * w * c] * 2


def test_psnr():
    from ngp_pl_amd import metrics
    p, t, _ = R.images("noise", 3, 13, 17, 3)
    same = metrics.psnr(dev(p), dev(p.copy()))
    assert same.dtype == torch.float64 and same.tolist() == [float("inf")] * 3
    want_sums, want_counts = R.sq_error_f32(p, t)
    for dr in (1.0, 255.0):
        got = metrics.psnr(dev(p), dev(t), data_range=dr).tolist()
        assert all(abs(a - R.psnr(s, k, dr)) < 1e-9 for a, s, k in zip(got, want_sums, want_counts))
    half = metrics.psnr(dev(p).half(), dev(t).half()).tolist()                                              # other float dtypes: converted to f32 first
    hs, hk = R.sq_error_f32(p.astype(np.float16).astype(F), t.astype(np.float16).astype(F))
    assert all(abs(a - R.psnr(s, k)) < 1e-9 for a, s, k in zip(half, hs, hk))


# ---- 4. refused calls


def test_refused_calls_return_their_status_and_leave_the_outputs_untouched():
    from ngp_pl_amd import _metrics_lib as L
    lib = L.lib()
    n, c, h, w = 1, 3, 20, 20
    p = torch.rand(n, h, w, c, device="cuda")
    t = torch.rand(n, h, w, c, device="cuda")
    nbytes = lib.ngp_metrics_workspace_bytes(n, c, h, w)
    ws = torch.zeros(nbytes // 8 + 8, dtype=torch.int64, device="cuda")
    total = torch.full((n,), -12345.5, dtype=torch.float64, device="cuda")
    count = torch.full((n,), -777, dtype=torch.int64, device="cuda")
    smap = torch.full((n, h, w, c), -3.25, dtype=torch.float32, device="cuda")           # larger than any map asked for below
    ok = dict(pred=p.data_ptr(), n=n, c=c, h=h, w=w, dr=1.0, wsb=nbytes)

    def ssim(**kw):
        a = dict(ok, **kw)
        return lib.ngp_metrics_ssim(a["pred"], t.data_ptr(), None, a["n"], a["c"], a["h"], a["w"], L.HWC, a["dr"], ws.data_ptr(), a["wsb"],
                                    total.data_ptr(), count.data_ptr(), smap.data_ptr(), L.stream())

    def sq(**kw):
        a = dict(ok, **kw)
        return lib.ngp_metrics_sq_error(a["pred"], t.data_ptr(), None, a["n"], a["c"], a["h"], a["w"], L.HWC, ws.data_ptr(), a["wsb"],
                                        total.data_ptr(), count.data_ptr(), L.stream())

    for kw in (dict(h=10), dict(c=5), dict(pred=None), dict(wsb=nbytes - 1), dict(dr=0.0)):
        assert ssim(**kw) == -1, kw
    for kw in (dict(c=5), dict(pred=None), dict(wsb=nbytes - 1), dict(h=0)):
        assert sq(**kw) == -1, kw
    assert ssim(h=16385) == -5 and sq(w=16385) == -5
    torch.cuda.synchronize()
    assert (total == -12345.5).all() and (count == -777).all() and (smap == -3.25).all() and (ws == 0).all()
    assert ssim() == 0 and sq() == 0                                                     # the same buffers, accepted
    torch.cuda.synchronize()
    assert count.tolist() == [c * h * w]


# ---- 5. the classes, as train.py uses torchmetrics'


def test_metric_classes_over_two_updates():
    from ngp_pl_amd import metrics
    g = np.random.RandomState(2)
    batches = [(g.rand(2, 3, 21, 30).astype(F), g.rand(2, 3, 21, 30).astype(F)), (g.rand(1, 3, 25, 23).astype(F), g.rand(1, 3, 25, 23).astype(F))]
    val_psnr = metrics.PeakSignalNoiseRatio(data_range=1)
    val_ssim = metrics.StructuralSimilarityIndexMeasure(data_range=1)
    se, k, scores = [], [], []
    for a, b in batches:
        val_psnr(dev(a), dev(b))
        val_ssim(dev(a), dev(b))
        s, cnt = R.sq_error_f32(a, b, None, "chw")
        se, k = se + s, k + cnt
        _, s, cnt = R.ssim_f32(a, b, 1.0, None, "chw")
        scores += [x / y for x, y in zip(s, cnt)]
    assert int(val_psnr.total) == sum(k) and abs(val_psnr.compute().item() - R.psnr(math.fsum(se), sum(k))) < 1e-9
    assert val_ssim.total == 3 and abs(val_ssim.compute().item() - sum(scores) / 3) < 1e-9
    val_psnr.reset()
    val_ssim.reset()
    a, b = batches[1]
    first = val_psnr(dev(a), dev(b)).item(), val_ssim(dev(a), dev(b)).item()
    assert abs(first[0] - R.psnr(se[2], k[2])) < 1e-9 and abs(first[1] - scores[2]) < 1e-9
    assert abs(val_psnr.compute().item() - first[0]) < 1e-12 and abs(val_ssim.compute().item() - first[1]) < 1e-12


# ---- 6. evaluate_frames, compare_renders and the CLI on a small model


def make_model(seed=3):
    from ngp_pl_amd.networks import NGP
    torch.manual_seed(seed)
    m = NGP(scale=0.5).cuda()
    m.register_training_buffers()
    return m


def test_evaluate_frames():
    from ngp_pl_amd import metrics, synthetic as syn
    model = make_model()
    W, H = 24, 20
    K, poses = syn.intrinsics(W, H), syn.hemisphere_poses(2, seed=1)
    targets = np.random.RandomState(4).rand(2, H, W, 3).astype(F)
    out = metrics.evaluate_frames(model, K, poses, (W, H), targets, return_frames=True)
    frames = out["frames"].cpu().numpy()
    assert frames.shape == (2, H, W, 3) and np.isfinite(frames).all()
    se, k = R.sq_error_f32(frames, targets)
    _, s, cnt = R.ssim_f32(frames, targets, 1.0)
    assert len(out["psnr"]) == len(out["ssim"]) == 2
    for i in range(2):
        assert abs(out["psnr"][i] - R.psnr(se[i], k[i])) < 1e-9 and abs(out["ssim"][i] - s[i] / cnt[i]) < 1e-9
    assert abs(out["psnr_mean"] - sum(out["psnr"]) / 2) < 1e-12 and abs(out["ssim_mean"] - sum(out["ssim"]) / 2) < 1e-12
    assert "frames" not in metrics.evaluate_frames(model, K, poses[:1], (W, H), targets[:1])


@pytest.fixture
def true_density(monkeypatch):
    """The model's density lattice replaced by the procedural scene's true density, so that the small mesh is the scene's."""
    from ngp_pl_amd import mesh, synthetic as syn

    def volume(model, resolution=512, bounds=None, chunk=0):
        nx, ny, nz = mesh._resolution(resolution)
        xyz = mesh.lattice_points((nx, ny, nz), mesh._bounds(model, bounds))
        return syn.density(xyz).view(nz, ny, nx).contiguous()

    monkeypatch.setattr(mesh, "density_volume", volume)


def same(a, b, tol=1e-9):
    """Equal numbers within tol, nan equal to nan and inf to inf, None to None; lists and dicts element by element."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k], tol) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y, tol) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) and math.isnan(a):
        return isinstance(b, float) and math.isnan(b)
    return a == b or abs(a - b) <= tol


def reference_record(rec, data_range=1.0):
    """The record of compare_renders from the images, ids, depths and opacities it returned, through the restatement."""
    image, field = rec["images"].cpu().numpy(), rec["field_images"].cpu().numpy()
    ids, opacity = rec["ids"].cpu().numpy(), rec["field_opacity"].cpu().numpy()
    n, H, W, _ = image.shape
    covered = ids >= 0
    both = covered & (opacity >= F(0.5))
    want = dict(cameras=n, width=W, height=H, per_camera={})
    for region, mask in (("all", None), ("covered", covered), ("covered_and_opaque", both)):
        m = None if mask is None else mask.astype(np.uint8)
        se, k = R.sq_error_f32(image, field, m)
        _, s, cnt = R.ssim_f32(image, field, data_range, m)
        want["psnr_" + region] = R.psnr(math.fsum(se), sum(k), data_range)
        want["ssim_" + region] = R.mean(math.fsum(s), sum(cnt))
        want["per_camera"][region] = dict(psnr=[R.psnr(a, b, data_range) for a, b in zip(se, k)], ssim=[R.mean(a, b) for a, b in zip(s, cnt)])
    total = n * H * W
    want.update(share_all=1.0, share_covered=int(covered.sum()) / total, share_covered_and_opaque=int(both.sum()) / total,
                share_field_opaque=int((opacity >= F(0.5)).sum()) / total)
    dz = (rec["depth"].cpu()[torch.from_numpy(both)] - rec["field_depth"].cpu()[torch.from_numpy(both)]).abs()
    want["depth_abs_difference_median"] = float(dz.median().item()) if dz.numel() else None
    return want


def test_compare_renders_and_the_cli_flag(true_density, tmp_path, capsys):
    from ngp_pl_amd import mesh, synthetic as syn
    model = make_model()
    res = 48
    textured = mesh.extract_mesh(model, res, keep_largest=1, simplify_voxels=2, texture=3)
    W = H = 32
    K, poses = syn.intrinsics(W), syn.hemisphere_poses(2, seed=1)
    rec = mesh.compare_renders(model, textured, K, poses, (W, H), return_images=True)
    tensors = ("images", "ids", "depth", "field_images", "field_opacity", "field_depth")
    assert rec["images"].shape == rec["field_images"].shape == (2, H, W, 3) and rec["ids"].shape == rec["field_opacity"].shape == (2, H, W)
    img, ids, depth = mesh.render_textured(textured, K, poses, (W, H), return_ids=True)
    assert torch.equal(img, rec["images"]) and torch.equal(ids, rec["ids"]) and 0.05 < rec["share_covered"] < 1
    numbers = {k: v for k, v in rec.items() if k not in tensors}
    want = reference_record(rec)
    assert numbers.keys() == want.keys()
    for key in want:
        if key.startswith("share_"):
            assert numbers[key] == want[key], key                                        # the shares are exact
        else:
            assert same(numbers[key], want[key]), (key, numbers[key], want[key])
    plain = mesh.compare_renders(model, textured, K, poses, (W, H))
    assert not set(tensors) & set(plain) and same(plain, numbers)
    # the CLI: the same record as one JSON line after the mesh's line, and in --score-out
    slim = {"model." + k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith(("density_grid", "grid_coords"))}
    ckpt, out, cams, score = (str(tmp_path / n) for n in ("slim.ckpt", "scene.obj", "cams.npz", "score.json"))
    torch.save(slim, ckpt)
    np.savez(cams, K=np.asarray(K, F), poses=np.asarray(poses, F), img_wh=np.asarray([W, H]))
    assert mesh.main(["--ckpt", ckpt, "--resolution", str(res), "--keep-largest", "1", "--simplify-voxels", "2", "--texture-texels", "3", "--out", out,
                      "--score-cameras", cams, "--score-out", score]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-2].startswith(out + ": ")
    got = json.loads(lines[-1])
    assert got.keys() == numbers.keys() and same(got, numbers, 1e-6) and same(json.loads(open(score).read()), got, 0.0)
    with pytest.raises(SystemExit):
        mesh.main(["--ckpt", ckpt, "--out", str(tmp_path / "m.ply"), "--score-cameras", cams])          # a PLY carries no texture to score
