"""Times and figures of the texture atlas made of charts (libngp_meshchart.so) on the decimated mesh of
tools/meshdecimate_bench.py: the marching-cubes mesh of the procedural scene's true density at `--resolution`^3 (threshold
SIGMA_INSIDE / 2), decimated to the face count that vertex clustering with cells of `--simplify-voxels` (2) voxels gives.
Times: ngp_meshchart_classify, ngp_meshchart_label (stage 0), ngp_meshchart_raster per stage (the owner map cleared inside the
timed call), ngp_meshchart_dilate, ngp_meshchart_texel_points over the whole atlas in chunks of 2^22 texels and
ngp_meshchart_render of `--cameras` (100) hemisphere_poses at `--image` (256) pixels, each between two HIP events, the median of
`--reps` (15) after `--warmup` (3) with min and max; chart_atlas's wall time with its host reads; beside libngp_meshatlas.so's
classify, texel_points and render at the same texel size.
Figures: charts and evicted faces per stage, the share of the edges between two classified faces that are seams (the two faces
lie in different charts), the share of texels owned and filled, the share of faces that are charts of their own, the split
vertex count a GLB needs; PSNR over the covered pixels of the renders of both atlases at `--texel-voxels` (1) voxel per texel,
baked from the scene's analytic colour, against the renders of a fine uniform bake at `--fine-texels` (32).  With --raw the same
figures (no times, no PSNR) for the mesh before the decimation as well.  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ngp_pl_amd import _meshatlas_lib as al, _meshchart_lib as cl, mesh, synthetic as syn
from ngp_pl_amd._lib import ptr, stream
from tools.meshatlas_bench import CHUNK, points_ms, psnr_covered, scene_colour
from tools.meshquadric_bench import HI, LO, event_ms, lattice


def figures(m, t, dbg):
    """The shares of one chart atlas (host arithmetic on the faces and the chart ids)."""
    f = m.faces.cpu().numpy().astype(np.int64)
    chart = t.face_chart.cpu().numpy()
    n_f = len(f)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    owner = np.tile(np.arange(n_f), 3)
    keep = chart[owner] >= 0
    key = e[keep, 0] * (int(f.max()) + 1) + e[keep, 1]
    order = np.argsort(key, kind="stable")
    key, owner = key[order], owner[keep][order]
    pair = np.nonzero(key[1:] == key[:-1])[0]                       # consecutive faces on one edge
    seams = int((chart[owner[pair]] != chart[owner[pair + 1]]).sum())
    sizes = np.bincount(chart[chart >= 0])
    split = int(len(np.unique(np.stack([np.repeat(chart, 3), f.reshape(-1)], 1)[np.repeat(chart, 3) >= 0], axis=0)))
    filled = float((t.texel_face >= 0).float().mean())
    ct = t.corner_texels.cpu().numpy().astype(np.int64)
    area2 = (ct[:, 1, 0] - ct[:, 0, 0]) * (ct[:, 2, 1] - ct[:, 0, 1]) - (ct[:, 1, 1] - ct[:, 0, 1]) * (ct[:, 2, 0] - ct[:, 0, 0])
    return dict(vertices=int(m.vertices.shape[0]), faces=n_f, width=t.width, height=t.height, charts=t.n_charts,
                charts_per_stage=list(t.charts_per_stage), evicted_per_stage=list(t.evicted_per_stage), faces_without_chart=int((chart < 0).sum()),
                faces_per_class=np.bincount(dbg["face_class"].cpu().numpy(), minlength=7).tolist(),
                shared_edges=int(len(pair)), seam_edges=seams, seam_share=seams / max(1, len(pair)),
                single_face_charts=int((sizes == 1).sum()), single_face_share=float((sizes == 1).sum()) / n_f,
                largest_chart_faces=int(sizes.max()), split_vertices=split,
                texels_filled_share=filled, texels_in_faces_share=float(area2.sum()) / 512.0 / (t.width * t.height))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--simplify-voxels", type=float, default=2.0)
    ap.add_argument("--texel-voxels", type=float, default=1.0)
    ap.add_argument("--pad", type=int, default=2)
    ap.add_argument("--fine-texels", type=int, default=32)
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--raw", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "meshchart_bench needs a GPU"
    res, voxel = a.resolution, 1.0 / (a.resolution - 1)
    unit = mesh._grid(voxel, None)[0]
    size, pad = float(np.float32(a.texel_voxels * voxel)), a.pad
    out = dict(resolution=res, texel_voxels=a.texel_voxels, pad=pad, fine_texels=a.fine_texels, cameras=a.cameras, image=a.image, warmup=a.warmup,
               reps=a.reps, voxel=voxel)
    vol = lattice(res, syn.density)
    export = mesh.marching_cubes(vol, syn.SIGMA_INSIDE / 2, (LO, HI))
    del vol
    if a.raw:
        t, dbg = mesh.chart_atlas(export, size, pad, return_debug=True)
        out["raw"] = figures(export, t, dbg)
        del t, dbg
    target = mesh.simplify_clusters(export, mesh._grid(a.simplify_voxels * voxel, None)[0], origin=LO).faces.shape[0]
    m = mesh.decimate(export, unit, target_faces=target)
    del export
    v, f, extra = mesh._check_mesh(m)
    normals = extra[0] if extra[0] is not None else mesh.vertex_normals(m)
    m = mesh.Mesh(v, f, normals)
    n_v, n_f = v.shape[0], f.shape[0]
    box = (LO, HI)
    b6 = mesh._box6(box)
    s = stream()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t, dbg = mesh.chart_atlas(m, size, pad, return_debug=True)
    torch.cuda.synchronize()
    out["chart_atlas_wall_ms"] = (time.perf_counter() - t0) * 1e3
    out["decimated"] = figures(m, t, dbg)
    charted = mesh.bake_texture(None, m, texel_size=size, charts=dict(pad=pad), color_fn=scene_colour, box=box)
    adaptive = mesh.bake_texture(None, m, texel_size=size, color_fn=scene_colour, box=box)
    ta = adaptive.texture
    out["adaptive"] = dict(width=ta.width, height=ta.height)

    # times: the chart atlas's calls on the final state
    lib = cl.lib()
    i32, u8, i64 = torch.int32, torch.uint8, torch.int64
    cls, off, vf = torch.empty(n_f, dtype=u8, device="cuda"), torch.empty(n_v + 1, dtype=i64, device="cuda"), torch.empty(3 * n_f, dtype=i32, device="cuda")
    cws = torch.empty(lib.ngp_meshchart_classify_workspace_bytes(n_v, n_f) // 8 + 1, dtype=i64, device="cuda")
    lws = torch.empty(lib.ngp_meshchart_label_workspace_bytes(n_f) // 8 + 1, dtype=i64, device="cuda")
    times = {}
    times["classify_ms"] = event_ms(lambda: cl.call("ngp_meshchart_classify", ptr(v), ptr(f), n_v, n_f, size, ptr(cls), ptr(off), ptr(vf), ptr(cws),
                                                    cws.numel() * 8, s), a.warmup, a.reps)
    active = (cls < cl.NO_CLASS).to(u8)
    lab, chart, cnt = torch.empty(n_f, dtype=i32, device="cuda"), torch.full((n_f,), -1, dtype=i32, device="cuda"), torch.zeros(2, dtype=i64, device="cuda")
    times["label_ms"] = event_ms(lambda: cl.call("ngp_meshchart_label", ptr(f), n_v, n_f, ptr(cls), ptr(active), ptr(off), ptr(vf), 1, 0, ptr(lab),
                                                 ptr(chart), ptr(cnt), ptr(lws), lws.numel() * 8, s), a.warmup, a.reps)
    assert int(cnt[0]) == t.charts_per_stage[0] and torch.equal(lab, dbg["labels"][0])
    owner, scratch = torch.empty(t.height, t.width, dtype=i32, device="cuda"), torch.empty(t.height, t.width, dtype=i32, device="cuda")
    lo = 0
    for stage, n in enumerate(t.charts_per_stage):
        if n:
            def raster(lo=lo, hi=lo + n):
                owner.fill_(-1)
                cl.call("ngp_meshchart_raster", ptr(v), ptr(f), n_v, n_f, size, ptr(t.face_chart), ptr(t.chart_rects), t.n_charts, lo, hi, pad,
                        t.width, t.height, ptr(owner), s)
            times["raster_stage%d_ms" % stage] = event_ms(raster, a.warmup, a.reps)
        lo += n
    times["fill_ms"] = event_ms(lambda: owner.fill_(-1), a.warmup, a.reps)
    times["dilate_ms"] = event_ms(lambda: cl.call("ngp_meshchart_dilate", ptr(owner), ptr(scratch), t.width, t.height, pad, s), a.warmup, a.reps)
    times["texel_points_ms"] = points_ms(lambda begin, count, buf: cl.call(
        "ngp_meshchart_texel_points", ptr(v), ptr(f), ptr(normals), n_v, n_f, ptr(t.corner_texels), t.width, t.height, ptr(t.texel_face), b6, begin,
        count, ptr(buf[0]), ptr(buf[1]), ptr(buf[2]), s), t.width * t.height, a.warmup, a.reps)
    host = mesh._counts_array(ta.counts)
    acls, aorder, acounts = torch.empty(n_f, dtype=u8, device="cuda"), torch.empty(n_f, dtype=i32, device="cuda"), torch.empty(16, dtype=i64, device="cuda")
    aws = torch.empty(al.lib().ngp_meshatlas_classify_workspace_bytes(n_f) // 8, dtype=i64, device="cuda")
    times["meshatlas_classify_ms"] = event_ms(lambda: al.call("ngp_meshatlas_classify", ptr(v), ptr(f), n_v, n_f, size, 0, 15, ptr(acls), ptr(aorder),
                                                              ptr(acounts), ptr(aws), aws.numel() * 8, s), a.warmup, a.reps)
    times["meshatlas_texel_points_ms"] = points_ms(lambda begin, count, buf: al.call(
        "ngp_meshatlas_texel_points", ptr(v), ptr(f), ptr(normals), n_v, n_f, ptr(ta.order), host, b6, begin, count, ptr(buf[0]), ptr(buf[1]),
        ptr(buf[2]), s), ta.width * ta.height, a.warmup, a.reps)
    K, poses, wh = syn.intrinsics(a.image), syn.hemisphere_poses(a.cameras, seed=1), (a.image, a.image)
    times["render_ms"] = event_ms(lambda: mesh.render_textured(charted, K, poses, wh), 1, max(3, a.reps // 3))
    times["meshatlas_render_ms"] = event_ms(lambda: mesh.render_textured(adaptive, K, poses, wh), 1, max(3, a.reps // 3))
    out["times"] = times

    # quality against a fine uniform bake
    fine = mesh.bake_texture(None, m, a.fine_texels, color_fn=scene_colour, box=box)
    out["fine"] = dict(width=fine.texture.width, height=fine.texture.height)
    reference, ids, _ = mesh.render_textured(fine, K, poses, wh, return_ids=True)
    covered = ids >= 0
    out["covered_share"] = float(covered.float().mean())
    out["psnr_charts"] = psnr_covered(mesh.render_textured(charted, K, poses, wh), reference, covered)
    out["psnr_adaptive"] = psnr_covered(mesh.render_textured(adaptive, K, poses, wh), reference, covered)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
