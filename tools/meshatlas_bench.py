"""Times and figures of the texture atlas with texel density by face size (libngp_meshatlas.so) on the decimated mesh of
tools/meshdecimate_bench.py: the marching-cubes mesh of the procedural scene's true density at `--resolution`^3 (threshold
SIGMA_INSIDE / 2), decimated to the face count that vertex clustering with cells of `--simplify-voxels` (2) voxels gives.
Times: ngp_meshatlas_classify, ngp_meshatlas_place, ngp_meshatlas_texel_points over the whole atlas in chunks of 2^22 texels and
ngp_meshatlas_render of `--cameras` (100) hemisphere_poses at `--image` (256) pixels, each between two HIP events, the median of
`--reps` (15) after `--warmup` (3) with min and max; beside libngp_meshtex.so's texel_points and render for the uniform atlas at
`--texels` (8); and fit_texel_size's wall time with its host reads.
Figures: the class counts and the atlas sizes; PSNR of the renders of the uniform atlas and of the adaptive atlas at
fit_texel_size to the uniform atlas's side, both baked from the scene's analytic colour, against the renders of a fine uniform
bake at `--fine-texels` (32) from the same cameras, over the covered pixels (ngp_pl_amd.metrics).  Prints one JSON line.
Needs a GPU."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ngp_pl_amd import _meshatlas_lib as al, _meshtex_lib as tl, mesh, metrics, synthetic as syn
from ngp_pl_amd._lib import ptr, stream
from tools.meshquadric_bench import HI, LO, event_ms, lattice

CHUNK = 1 << 22


def scene_colour(p, d):
    return syn.colour(p)


def points_ms(call, total, warmup, reps):
    """All texels in chunks of CHUNK through `call(begin, count, buffers)`."""
    n = min(CHUNK, total)
    buf = (torch.empty(n, 3, device="cuda"), torch.empty(n, 3, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"))

    def run():
        for begin in range(0, total, CHUNK):
            call(begin, min(CHUNK, total - begin), buf)
    return event_ms(run, warmup, reps)


def psnr_covered(image, reference, covered):
    """PSNR over the covered pixels of all cameras: sums and counts pooled."""
    se, n = metrics.sq_error(image, reference, covered)
    return float(-10.0 * torch.log10(se.sum() / n.sum().double()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--simplify-voxels", type=float, default=2.0)
    ap.add_argument("--texels", type=int, default=8)
    ap.add_argument("--fine-texels", type=int, default=32)
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "meshatlas_bench needs a GPU"
    res, voxel = a.resolution, 1.0 / (a.resolution - 1)
    unit = mesh._grid(voxel, None)[0]
    out = dict(resolution=res, texels=a.texels, fine_texels=a.fine_texels, cameras=a.cameras, image=a.image, warmup=a.warmup, reps=a.reps, voxel=voxel)
    vol = lattice(res, syn.density)
    export = mesh.marching_cubes(vol, syn.SIGMA_INSIDE / 2, (LO, HI))
    del vol
    target = mesh.simplify_clusters(export, mesh._grid(a.simplify_voxels * voxel, None)[0], origin=LO).faces.shape[0]
    m = mesh.decimate(export, unit, target_faces=target)
    del export
    v, f, extra = mesh._check_mesh(m)
    normals = extra[0] if extra[0] is not None else mesh.vertex_normals(m)
    m = mesh.Mesh(v, f, normals)
    n_v, n_f = v.shape[0], f.shape[0]
    out.update(vertices=n_v, faces=n_f)
    box = (LO, HI)
    b6 = mesh._box6(box)
    s = stream()

    uniform = mesh.bake_texture(None, m, a.texels, color_fn=scene_colour, box=box)
    side = max(uniform.texture.width, uniform.texture.height)
    t0 = time.perf_counter()
    size = mesh.fit_texel_size(m, side)
    torch.cuda.synchronize()
    out["fit_texel_size_wall_ms"] = (time.perf_counter() - t0) * 1e3
    adaptive = mesh.bake_texture(None, m, texel_size=size, color_fn=scene_colour, box=box)
    t = adaptive.texture
    out["uniform"] = dict(width=uniform.texture.width, height=uniform.texture.height)
    out["adaptive"] = dict(width=t.width, height=t.height, texel_size=size, texel_size_voxels=size / voxel,
                           faces_per_texels={str(T): c for T, c in zip(al.LADDER, t.counts) if c})

    # times: the adaptive atlas's calls
    cls = torch.empty(n_f, dtype=torch.uint8, device="cuda")
    order = torch.empty(n_f, dtype=torch.int32, device="cuda")
    counts = torch.empty(16, dtype=torch.int64, device="cuda")
    ws_bytes = al.lib().ngp_meshatlas_classify_workspace_bytes(n_f)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device="cuda")
    place = torch.empty(n_f, 2, dtype=torch.int32, device="cuda")
    host = mesh._counts_array(t.counts)
    times = {}
    times["classify_ms"] = event_ms(lambda: al.call("ngp_meshatlas_classify", ptr(v), ptr(f), n_v, n_f, size, 0, 15, ptr(cls), ptr(order), ptr(counts),
                                                    ptr(ws), ws_bytes, s), a.warmup, a.reps)
    assert counts.tolist() == list(t.counts) and torch.equal(order, t.order)
    times["place_ms"] = event_ms(lambda: al.call("ngp_meshatlas_place", ptr(order), host, n_f, ptr(place), s), a.warmup, a.reps)
    times["texel_points_ms"] = points_ms(lambda begin, count, buf: al.call(
        "ngp_meshatlas_texel_points", ptr(v), ptr(f), ptr(normals), n_v, n_f, ptr(order), host, b6, begin, count, ptr(buf[0]), ptr(buf[1]), ptr(buf[2]), s),
        t.width * t.height, a.warmup, a.reps)
    times["meshtex_texel_points_ms"] = points_ms(lambda begin, count, buf: tl.call(
        "ngp_meshtex_texel_points", ptr(v), ptr(f), ptr(normals), n_v, n_f, a.texels, b6, begin, count, ptr(buf[0]), ptr(buf[1]), ptr(buf[2]), s),
        uniform.texture.width * uniform.texture.height, a.warmup, a.reps)
    K, poses, wh = syn.intrinsics(a.image), syn.hemisphere_poses(a.cameras, seed=1), (a.image, a.image)
    times["render_ms"] = event_ms(lambda: mesh.render_textured(adaptive, K, poses, wh), 1, max(3, a.reps // 3))
    times["meshtex_render_ms"] = event_ms(lambda: mesh.render_textured(uniform, K, poses, wh), 1, max(3, a.reps // 3))
    out["times"] = times

    # quality against a fine uniform bake
    fine = mesh.bake_texture(None, m, a.fine_texels, color_fn=scene_colour, box=box)
    out["fine"] = dict(width=fine.texture.width, height=fine.texture.height)
    reference, ids, _ = mesh.render_textured(fine, K, poses, wh, return_ids=True)
    covered = ids >= 0
    out["covered_share"] = float(covered.float().mean())
    out["psnr_uniform"] = psnr_covered(mesh.render_textured(uniform, K, poses, wh), reference, covered)
    out["psnr_adaptive"] = psnr_covered(mesh.render_textured(adaptive, K, poses, wh), reference, covered)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
