"""Times and figures of the texture bake from photographs (libngp_meshphoto.so) on the decimated mesh of
tools/meshdecimate_bench.py: the marching-cubes mesh of the procedural scene's true density at `--resolution`^3 (threshold
SIGMA_INSIDE / 2), decimated to the face count that vertex clustering with cells of `--simplify-voxels` (2) voxels gives, with the
adaptive atlas that fit_texel_size finds for `--max-side` (4096) texels.  The photographs are the scene's ground-truth renders
(synthetic.render_ground_truth) from `--cameras` (100) hemisphere_poses at `--image` (256) pixels, stored as bytes.
Times: ngp_meshphoto_accumulate over the whole atlas in chunks of 2^22 texels against all the cameras at once, ngp_meshphoto_resolve
over the whole atlas, and the depth buffers of the cameras (ngp_meshcull_views), each between two HIP events, the median of `--reps`
(5) after `--warmup` (1) with min and max; beside them the field's colour forward (an NGP model of the default size, untrained: the
time does not depend on the weights) over the same texels in bake_texture's chunks of 2^20, and the wall time of the two whole
bakes, bake_texture and bake_texture_from_images.
Figures: the share of valid texels the photographs colour; PSNR and SSIM (ngp_pl_amd.metrics, pooled over the frames) of
render_textured against `--held-out` (10) ground-truth frames from other cameras, for the field bake (the scene's analytic colour
at the texel points, seen along minus the normal, which is what bake_texture asks a perfect field) and for the photo bake (the same
analytic colour where no photograph sees a texel).  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ngp_pl_amd import _meshphoto_lib as pl, mesh, metrics, synthetic as syn
from ngp_pl_amd._lib import ptr, stream
from tools.meshquadric_bench import HI, LO, event_ms, lattice

CHUNK = 1 << 22
FIELD_CHUNK = 1 << 20
RAYS = 1 << 16


class AnalyticField(torch.nn.Module):
    """The procedural scene as a colour field with the model's call: (sigma, rgb) at points seen along unit directions."""
    xyz_min, xyz_max = torch.tensor(LO), torch.tensor(HI)

    def forward(self, p, d):
        return syn.density(p), syn.colour(p, d)


def ground_truth(K, poses, size):
    """(C, size, size, 3) f32 frames of the scene, a camera at a time, RAYS rays at a time."""
    dirs = syn.get_ray_directions(size, size, K, device="cuda")
    frames = torch.empty(len(poses), size * size, 3, device="cuda")
    for c, pose in enumerate(poses):
        ro, rd = syn.get_rays(dirs, torch.as_tensor(pose, dtype=torch.float32).cuda())
        for b in range(0, size * size, RAYS):
            frames[c, b:b + RAYS] = syn.render_ground_truth(ro[b:b + RAYS].contiguous(), rd[b:b + RAYS].contiguous())[0]
    return frames.view(len(poses), size, size, 3)


def score(m, K, poses, wh, target):
    image = mesh.render_textured(m, K, poses, wh)
    se, n = metrics.sq_error(image, target)
    ss, ns = metrics.ssim_sums(image, target)
    return dict(psnr=float(-10.0 * torch.log10(se.sum() / n.sum().double())), ssim=float(ss.sum() / ns.sum().double()))


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--simplify-voxels", type=float, default=2.0)
    ap.add_argument("--max-side", type=int, default=4096)
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--held-out", type=int, default=10)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--guard", type=int, default=1)
    ap.add_argument("--min-cos", type=float, default=0.1)
    ap.add_argument("--power", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "meshphoto_bench needs a GPU"
    res, voxel = a.resolution, 1.0 / (a.resolution - 1)
    unit = mesh._grid(voxel, None)[0]
    bias = 2.0 * voxel
    out = dict(resolution=res, max_side=a.max_side, cameras=a.cameras, held_out=a.held_out, image=a.image, bias=bias, guard=a.guard, min_cos=a.min_cos,
               power=a.power, warmup=a.warmup, reps=a.reps, voxel=voxel)
    vol = lattice(res, syn.density)
    export = mesh.marching_cubes(vol, syn.SIGMA_INSIDE / 2, (LO, HI))
    del vol
    target = mesh.simplify_clusters(export, mesh._grid(a.simplify_voxels * voxel, None)[0], origin=LO).faces.shape[0]
    m = mesh.decimate(export, unit, target_faces=target)
    del export
    v, f, extra = mesh._check_mesh(m)
    normals = extra[0] if extra[0] is not None else mesh.vertex_normals(m)
    m = mesh.Mesh(v, f, normals)
    out.update(vertices=v.shape[0], faces=f.shape[0])
    box = (LO, HI)
    size = mesh.fit_texel_size(m, a.max_side)
    t = mesh.texture_atlas(m, texel_size=size)
    n = t.width * t.height
    out["atlas"] = dict(width=t.width, height=t.height, texel_size=size, texel_size_voxels=size / voxel)

    wh = (a.image, a.image)
    K, poses, held = syn.intrinsics(a.image), syn.hemisphere_poses(a.cameras, seed=1), syn.hemisphere_poses(a.held_out, seed=2)
    photos = (ground_truth(K, poses, a.image) * 255.0).round().to(torch.uint8)
    truth = ground_truth(K, held, a.image)
    Kd, Pd, W, H = mesh._cameras(K, poses, wh, v.device)

    # times: the depth buffers, accumulate over the whole atlas, resolve
    s = stream()
    times = {}
    times["depth_buffers_ms"] = event_ms(lambda: mesh._views(v, f, Kd, Pd, wh, bias, mesh.NEAR_DISTANCE, 4 * W * H * a.cameras), a.warmup, a.reps)
    zbuf = mesh._views(v, f, Kd, Pd, wh, bias, mesh.NEAR_DISTANCE, 4 * W * H * a.cameras)[1]
    points, dirs, valid = mesh.texel_points(m, t, box)
    acc = torch.zeros(n, 4, device="cuda")
    views = torch.zeros(n, dtype=torch.int32, device="cuda")
    rgb = torch.empty(n, 3, device="cuda")
    seen = torch.empty(n, dtype=torch.uint8, device="cuda")

    def accumulate():
        for b in range(0, n, CHUNK):
            c = min(CHUNK, n - b)
            pl.call("ngp_meshphoto_accumulate", ptr(points[b:]), ptr(dirs[b:]), ptr(valid[b:]), c, ptr(Kd), ptr(Pd), a.cameras, W, H, ptr(photos),
                    ptr(zbuf), mesh.NEAR_DISTANCE, bias, a.guard, a.min_cos, a.power, ptr(acc[b:]), ptr(views[b:]), s)

    times["accumulate_ms"] = event_ms(accumulate, a.warmup, a.reps)
    acc.zero_()
    views.zero_()
    accumulate()
    times["resolve_ms"] = event_ms(lambda: pl.call("ngp_meshphoto_resolve", ptr(acc), ptr(views), ptr(valid), n, 1, ptr(rgb), ptr(seen), s), a.warmup, a.reps)
    n_valid, n_seen = int(valid.sum()), int(seen.sum())
    out.update(texels=n, valid_texels=n_valid, seen_texels=n_seen, seen_share=n_seen / max(n_valid, 1), pairs=n_valid * a.cameras,
               mean_views_of_seen=float(views[seen == 1].float().mean()) if n_seen else 0.0)

    # beside them: the field's colour forward over the same texels, and the two whole bakes
    from ngp_pl_amd.networks import NGP
    model = NGP(scale=0.5).cuda()

    def field():
        with torch.no_grad():
            for b in range(0, n, FIELD_CHUNK):
                model(points[b:b + FIELD_CHUNK], dirs[b:b + FIELD_CHUNK])
    times["field_forward_ms"] = event_ms(field, a.warmup, a.reps)
    del acc, views, rgb, seen, points, dirs, valid
    _, times["bake_texture_wall_ms"] = wall_ms(lambda: mesh.bake_texture(model, m, texel_size=size))
    cam = dict(images=photos, K=K, poses=poses, img_wh=wh, bias=bias, guard=a.guard, min_cos=a.min_cos, power=a.power)
    _, times["bake_texture_from_images_wall_ms"] = wall_ms(lambda: mesh.bake_texture_from_images(m, texel_size=size, box=box, **cam))
    out["times"] = times

    # quality against held-out ground truth
    field_bake = mesh.bake_texture(AnalyticField(), m, texel_size=size)
    photo_bake = mesh.bake_texture_from_images(m, texel_size=size, model=AnalyticField(), **cam)
    out["field_bake"] = score(field_bake, K, held, wh, truth)
    out["photo_bake"] = score(photo_bake, K, held, wh, truth)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
