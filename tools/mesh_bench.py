"""Mesh export timing on the trained procedural scene: trains `--steps` native steps, then times extract_mesh at `--resolution`
(wall time with a device sync, split into density volume and marching cubes; best of `--reps`) and prints one JSON line with V, F
and the marching cubes' algorithmic bytes (volume read twice + outputs).  Under `rocprofv3 --kernel-trace --stats` the kernel
times of the same extraction divide those bytes (rate / 8 TB/s = share of HBM peak).

The component filter is timed on that mesh: connected_components, then filter_components(keep_largest=1) (which labels again),
each wall time with a device sync, best of `--reps`; V, F and the component count C before and after.  `--surface-stats N` adds, at
resolution N, the component count, the largest component's share of the faces and the vertices' distance to the analytic surface
(median / p95 in voxels) before and after keep_largest=1.

The visibility cull is timed on the same mesh: cull_invisible against `--cull-cameras` synthetic.hemisphere_poses at
`--cull-size`^2 pixels with a bias of two voxels, wall time with a device sync, best of `--reps`; V and F kept.  With
`--surface-stats N` the vertex-to-surface median / p95 of the N^3 mesh after the cull for min_views = 1, 5, 25 and 50 of the cameras
(vertices kept, median, p95 per row), and after keep_largest=1 followed by the cull.

The simplification is timed on the same mesh: simplify_clusters with cells of K = 2 and K = 4 voxels from the box's lower corner
(as extract_mesh(simplify_voxels=K) calls it), wall time with a device sync, best of `--reps`; V and F before and after.  With
`--surface-stats N` the vertex-to-surface median / p95 of the N^3 mesh after each.

The smoothing is timed on the same mesh, on the grid of one voxel from the box's lower corner (as extract_mesh(smooth=...) calls
it): ngp_meshsmooth_topology (the edge table, the degrees and the neighbour lists), ten Taubin pairs (twenty gather passes) on
those lists, and vertex_normals, each wall time with a device sync, best of `--reps`; the edge count and the free vertices.  For
scale, the same ten pairs as torch.index_add_ of float32 positions over the same directed edges (built outside the timing).

`--tsdf` adds the depth-map fusion: render_depths of the `--cull-cameras` hemisphere poses at `--cull-size`^2 pixels and tsdf_volume
of them at `--resolution` with a truncation of 4 voxels, each wall time with a device sync, best of `--reps`; the integrator's
algorithmic bytes (the 12-byte state read and written once, one 4-byte depth per (point, camera) pair that reaches the gather) and
the number of those pairs.  With `--surface-stats N` V, F, the component count, the largest component's share and the
vertex-to-surface median / p95 of the N^3 mesh of extract_mesh(tsdf=...) (trunc_voxels 4, min_opacity 0.5), and again after
keep_largest=1.

`--texture` adds the texture atlas: on the mesh simplified at K = 2, with `--texture-texels` (8) texels per face leg, the wall times
with a device sync (best of `--reps`) of bake_texture, split into the texel points (ngp_meshtex_texel_points over the whole atlas)
and the field evaluation with the quantisation (the rest), of render_textured for the `--cull-cameras` hemisphere poses at
`--cull-size`^2 pixels, and the PSNR and SSIM (mesh.compare_renders, with its wall time) of those renders against the field's own
test-time render() from the same cameras (both on a white background), over all pixels, over the pixels the mesh covers, and over
those of them where the field's render is opaque too (opacity >= 0.5), with the shares of the pixels in each set, and over the
last set the median absolute difference between the mesh's depth and the field's (depth / opacity), in world units."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ngp_pl_amd import mesh, synthetic as syn
from ngp_pl_amd.networks import NGP
from ngp_pl_amd.trainer import Trainer


def batch(n, seed, W=200):
    g = np.random.RandomState(seed)
    dirs = syn.get_ray_directions(W, W, syn.intrinsics(W))
    poses = syn.hemisphere_poses(16, seed=1)
    ro, rd = syn.get_rays(dirs[torch.from_numpy(g.randint(0, W * W, n))], poses[torch.from_numpy(g.randint(0, 16, n))])
    ro, rd = ro.cuda().contiguous(), rd.cuda().contiguous()
    gt, _ = syn.render_ground_truth(ro, rd, n_steps=192)
    return ro, rd, gt.contiguous()


def surface_error(m, n):
    """|signed distance - iso distance| of the vertices, in voxels of an n^3 lattice over the unit box: median, p95."""
    p = 20.0 / syn.SIGMA_INSIDE
    sd_iso = -syn.EDGE * math.log(p / (1 - p))
    d = (syn.signed_distance(m.vertices.double()) - sd_iso).abs() * (n - 1)
    return d.median().item(), torch.quantile(d[torch.randperm(len(d), device=d.device)[:1000000]], 0.95).item()


def best_of(reps, fn):
    best, out = None, None
    for _ in range(reps + 1):                         # the first round warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    return best, out


def smoothing(m, cell, lo, reps):
    """Times of the three calls of libngp_meshsmooth.so on mesh m, and of ten pairs done with torch.index_add_ in float32."""
    from ngp_pl_amd import _meshsmooth_lib as L
    v, f, _ = mesh._check_mesh(m)
    cell, _ = mesh._grid(cell, None)
    t_topology, (degree, flags, totals, ws, ws_bytes, o) = best_of(reps, lambda: mesh._topology(v, f, cell, lo, True))
    out = torch.empty_like(v)

    def pairs():
        with L.device_guard(v.device):
            L.call("ngp_meshsmooth_taubin", L.ptr(v), v.shape[0], f.shape[0], L.ptr(o), cell, 10, 0.5, -0.53, L.ptr(ws), ws_bytes, L.ptr(out), L.stream())

    t_pairs, _ = best_of(reps, pairs)
    t_normals, _ = best_of(reps, lambda: mesh.vertex_normals(mesh.Mesh(out, f)))
    # the same edges and the same free vertices, float32 positions, one index_add_ per pass
    fl = f.long()
    e = torch.cat([fl[:, [0, 1]], fl[:, [1, 2]], fl[:, [2, 0]]])
    e = torch.unique(torch.cat([e, e.flip(1)]), dim=0)
    src, dst = e[:, 0].contiguous(), e[:, 1].contiguous()
    free = ((flags & 4) != 0).unsqueeze(1)
    deg = degree.clamp(min=1).float().unsqueeze(1)

    def eager():
        x = v
        for _ in range(10):
            for factor in (0.5, -0.53):
                s = torch.zeros_like(x).index_add_(0, dst, x[src])
                x = torch.where(free, x + factor * (s / deg - x), x)
        return x

    t_eager, x = best_of(reps, eager)
    n_edges, n_boundary, n_free, _ = totals.tolist()
    return dict(smooth_topology_s=t_topology, smooth_10_pairs_s=t_pairs, smooth_normals_s=t_normals, smooth_10_pairs_index_add_f32_s=t_eager,
                smooth_edges=n_edges, smooth_boundary_edges=n_boundary, smooth_free_vertices=n_free, smooth_max_degree=int(degree.max().item()),
                smooth_max_abs_difference_to_index_add_voxels=float((x - out).abs().max().item() / cell))


def texturing(model, m, texels, K, poses, wh, reps):
    """Times of bake_texture (texel points / field evaluation) and render_textured on mesh m, and mesh.compare_renders' PSNR and
    SSIM against render() with its wall time (both renders of every camera included)."""
    v, f, extra = mesh._check_mesh(m)
    t_atlas, tex = best_of(reps, lambda: mesh.texture_atlas(m, texels))
    n = tex.width * tex.height
    b6 = mesh._box6(mesh._box(model))
    t_points, (_, _, ok) = best_of(reps, lambda: mesh._texel_points(v, f, extra[0], tex, b6, 0, n))
    n_valid = int(ok.sum().item())
    del ok
    t_bake, baked = best_of(reps, lambda: mesh.bake_texture(model, m, texels))
    t_render, images = best_of(reps, lambda: mesh.render_textured(baked, K, poses, wh, return_ids=True))
    del images
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    score = mesh.compare_renders(model, baked, K, poses, wh)                     # renders both, scores on the device, one host read
    t_compare = time.perf_counter() - t0
    W = wh[0]
    return dict(texture_texels=texels, texture_width=tex.width, texture_height=tex.height, texture_texels_total=n, texture_texels_valid=n_valid,
                texture_faces=f.shape[0], texture_atlas_s=t_atlas, texture_texel_points_s=t_points, bake_texture_s=t_bake,
                bake_field_evaluation_s=t_bake - t_points - t_atlas, render_textured_s=t_render, render_cameras=len(poses), render_size=W,
                render_covered_share=score["share_covered"], render_field_opaque_share=score["share_field_opaque"],
                render_covered_and_opaque_share=score["share_covered_and_opaque"],
                psnr_vs_field_render_db=score["psnr_all"], psnr_vs_field_render_covered_db=score["psnr_covered"],
                psnr_vs_field_render_covered_and_opaque_db=score["psnr_covered_and_opaque"],
                ssim_vs_field_render=score["ssim_all"], ssim_vs_field_render_covered=score["ssim_covered"],
                ssim_vs_field_render_covered_and_opaque=score["ssim_covered_and_opaque"], compare_renders_s=t_compare,
                depth_abs_difference_to_field_median=score["depth_abs_difference_median"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=20.0)
    ap.add_argument("--surface-stats", type=int, default=0, metavar="N", help="also report the filter's effect on the N^3 mesh")
    ap.add_argument("--cull-cameras", type=int, default=100, metavar="C", help="cameras of the visibility cull")
    ap.add_argument("--cull-size", type=int, default=800, metavar="W", help="image width and height of the visibility cull")
    ap.add_argument("--tsdf", action="store_true", help="also time render_depths and tsdf_volume, and report the TSDF mesh under --surface-stats")
    ap.add_argument("--texture", action="store_true", help="also time bake_texture and render_textured on the K = 2 mesh, with the PSNR against render()")
    ap.add_argument("--texture-texels", type=int, default=8, metavar="T", help="texels per face leg of --texture")
    a = ap.parse_args()
    torch.manual_seed(2)
    model = NGP(scale=0.5).cuda()
    model.register_training_buffers()
    tr = Trainer(model)
    bs = [batch(4096, 500 + i) for i in range(16)]
    for it in range(a.steps):
        tr.step(*bs[it % 16], next_batch=bs[(it + 1) % 16][:2])
    torch.cuda.synchronize()
    n = a.resolution
    res = dict(resolution=n, steps=a.steps)
    best = None
    for _ in range(a.reps + 1):                       # the first round warms up (code objects, allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vol = mesh.density_volume(model, n)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lo, hi = mesh._box(model)
        m = mesh.marching_cubes(vol, a.threshold, (lo, hi))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        del vol
        cur = (t2 - t0, t1 - t0, t2 - t1)
        best = cur if best is None or cur[0] < best[0] else best
    V, F = m.vertices.shape[0], m.faces.shape[0]
    res.update(total_s=best[0], density_volume_s=best[1], marching_cubes_s=best[2], V=V, F=F,
               mc_algorithmic_bytes=2 * 4 * n ** 3 + V * 24 + F * 12)
    t_label, comps = best_of(a.reps, lambda: mesh.connected_components(m))
    t_filter, kept = best_of(a.reps, lambda: mesh.filter_components(m, keep_largest=1))
    res.update(connected_components_s=t_label, filter_keep_largest_1_s=t_filter, C=comps.n_components,
               V_kept=kept.vertices.shape[0], F_kept=kept.faces.shape[0], C_kept=mesh.connected_components(kept).n_components)
    K, poses, wh = syn.intrinsics(a.cull_size), syn.hemisphere_poses(a.cull_cameras, seed=1), (a.cull_size, a.cull_size)
    t_cull, seen = best_of(a.reps, lambda: mesh.cull_invisible(m, K, poses, wh, 2.0 / (n - 1)))
    res.update(cull_invisible_s=t_cull, cull_cameras=a.cull_cameras, cull_size=a.cull_size, V_seen=seen.vertices.shape[0], F_seen=seen.faces.shape[0])
    for k in (2, 4):
        t_simplify, small = best_of(a.reps, lambda: mesh.simplify_clusters(m, k * max((h - l) / (n - 1) for l, h in zip(lo, hi)), origin=lo))
        res.update({"simplify_k%d_s" % k: t_simplify, "V_simplified_k%d" % k: small.vertices.shape[0], "F_simplified_k%d" % k: small.faces.shape[0]})
    res.update(smoothing(m, max((h - l) / (n - 1) for l, h in zip(lo, hi)), lo, a.reps))
    if a.texture:
        small = mesh.simplify_clusters(m, 2 * max((h - l) / (n - 1) for l, h in zip(lo, hi)), origin=lo)
        res.update(texturing(model, small, a.texture_texels, K, poses, wh, min(a.reps, 2)))
    depths = None
    if a.tsdf:
        t_depths, depths = best_of(min(a.reps, 1), lambda: mesh.render_depths(model, K, poses, wh))
        trunc = 4.0 * max((h - l) / (n - 1) for l, h in zip(lo, hi))
        t_tsdf, _ = best_of(a.reps, lambda: mesh.tsdf_volume(n, (lo, hi), K, poses, wh, depths, trunc))
        _, _, seen_n, behind_n = mesh.tsdf_volume(n, (lo, hi), K, poses, wh, depths, trunc, return_state=True)
        pairs = int(seen_n.sum(dtype=torch.int64).item() + behind_n.sum(dtype=torch.int64).item())
        del seen_n, behind_n
        res.update(render_depths_s=t_depths, tsdf_volume_s=t_tsdf, tsdf_pairs=n ** 3 * a.cull_cameras, tsdf_gather_pairs=pairs,
                   tsdf_algorithmic_bytes=2 * 12 * n ** 3 + 4 * pairs, depth_pixels_finite=int(torch.isfinite(depths).sum().item()))
    if a.surface_stats:
        ns = a.surface_stats
        ms = mesh.extract_mesh(model, ns, a.threshold)
        cs = mesh.connected_components(ms)
        mk = mesh.filter_components(ms, keep_largest=1)
        before, after = surface_error(ms, ns), surface_error(mk, ns)
        mc, mkc = [mesh.cull_invisible(x, K, poses, wh, 2.0 / (ns - 1)) for x in (ms, mk)]
        culled, both = surface_error(mc, ns), surface_error(mkc, ns)
        by_min_views = {}
        for mv in (1, 5, 25, 50):
            x = mesh.cull_invisible(ms, K, poses, wh, 2.0 / (ns - 1), min_views=mv)
            by_min_views[mv] = (x.vertices.shape[0],) + (surface_error(x, ns) if x.vertices.shape[0] else (None, None))
        simplified = {}
        for k in (2, 4):
            x = mesh.simplify_clusters(ms, k * max((h - l) / (ns - 1) for l, h in zip(lo, hi)), origin=lo)
            simplified[k] = (x.vertices.shape[0], x.faces.shape[0]) + (surface_error(x, ns) if x.vertices.shape[0] else (None, None))
        res.update(surface=dict(resolution=ns, simplified_by_voxels=simplified, V=ms.vertices.shape[0], F=ms.faces.shape[0], C=cs.n_components,
                                largest_face_share=cs.faces_per_component.max().item() / ms.faces.shape[0],
                                faces_per_component_top5=torch.sort(cs.faces_per_component, descending=True).values[:5].tolist(),
                                V_kept=mk.vertices.shape[0], F_kept=mk.faces.shape[0],
                                median_voxels=before[0], p95_voxels=before[1], median_voxels_kept=after[0], p95_voxels_kept=after[1],
                                V_seen=mc.vertices.shape[0], F_seen=mc.faces.shape[0], median_voxels_seen=culled[0], p95_voxels_seen=culled[1],
                                V_kept_seen=mkc.vertices.shape[0], F_kept_seen=mkc.faces.shape[0], median_voxels_kept_seen=both[0],
                                p95_voxels_kept_seen=both[1], seen_by_min_views=by_min_views))
        if a.tsdf:
            mt = mesh.extract_mesh(model, ns, tsdf=dict(K=K, poses=poses, img_wh=wh, trunc_voxels=4.0, min_opacity=0.5, depths=depths))
            ct = mesh.connected_components(mt)
            mtk = mesh.filter_components(mt, keep_largest=1)
            e, ek = surface_error(mt, ns), surface_error(mtk, ns)
            res["surface"].update(tsdf=dict(V=mt.vertices.shape[0], F=mt.faces.shape[0], C=ct.n_components,
                                            largest_face_share=ct.faces_per_component.max().item() / mt.faces.shape[0],
                                            median_voxels=e[0], p95_voxels=e[1], V_kept=mtk.vertices.shape[0], F_kept=mtk.faces.shape[0],
                                            median_voxels_kept=ek[0], p95_voxels_kept=ek[1]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
