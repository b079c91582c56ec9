"""Times and figures of the normal-map bake (libngp_meshnormal.so) on the decimated mesh of tools/meshdecimate_bench.py: the
marching-cubes mesh of the procedural scene's true density at `--resolution`^3 (threshold SIGMA_INSIDE / 2) is the detail mesh;
the simplified mesh is its decimation to the face count that vertex clustering with cells of `--simplify-voxels` (2) voxels
gives, with the adaptive atlas that fit_texel_size finds for `--max-side` (4096) texels.
Times (wall time with a device sync, `--warmup` (2) calls, the median of `--reps` (7) with min and max): transfer_normals on the
atlas's VALID texels, gathered into arrays of their own, against a grid built beforehand; beside it
closest_on_mesh(return_points=True) on the same points and the same grid, the kernel this one was derived from, so that both do
the same work; the grid build; the whole bake_normal_map; and bake_texture with an NGP model of the
default size (untrained: the time does not depend on the weights).
Figures: the share of valid texels that find a face; the angular error, in float64, of the decoded u8 map against the normalised
central-difference gradient of synthetic.signed_distance at the texel points, and beside it the same error for the simplified
mesh's interpolated vertex normals (the texels' own normals) and for its face normals.  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ngp_pl_amd import mesh, synthetic as syn
from tools.meshquadric_bench import HI, LO, lattice


def wall_ms(fn, warmup, reps):
    """(median, min, max) milliseconds of fn, a device sync on either side."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def true_normals(points, h):
    """The normalised central-difference gradient of the scene's signed distance at points (n, 3), float64, step h."""
    p = points.double()
    g = torch.empty_like(p)
    for k in range(3):
        e = torch.zeros(3, dtype=torch.float64, device=p.device)
        e[k] = h
        g[:, k] = (syn.signed_distance(p + e) - syn.signed_distance(p - e)) / (2.0 * h)
    return g / g.norm(dim=1, keepdim=True)


def angle_stats(a, b, keep):
    """mean, median, 95th percentile and max of the angle in degrees between the rows of a and b (float64) where keep."""
    a, b = a.double()[keep], b.double()[keep]
    a, b = a / a.norm(dim=1, keepdim=True), b / b.norm(dim=1, keepdim=True)
    deg = torch.rad2deg(torch.atan2(torch.linalg.cross(a, b).norm(dim=1), (a * b).sum(1)))
    deg = deg[torch.isfinite(deg)]
    return dict(mean=float(deg.mean()), median=float(deg.median()), p95=float(deg.kthvalue(max(1, int(0.95 * deg.numel()))).values), max=float(deg.max()),
                texels=int(deg.numel()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--simplify-voxels", type=float, default=2.0)
    ap.add_argument("--max-side", type=int, default=4096)
    ap.add_argument("--max-dist-voxels", type=float, default=None, help="default: max(4, 2 * simplify-voxels)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "meshnormal_bench needs a GPU"
    res, voxel = a.resolution, 1.0 / (a.resolution - 1)
    unit = mesh._grid(voxel, None)[0]
    reach = (a.max_dist_voxels if a.max_dist_voxels is not None else max(4.0, 2.0 * a.simplify_voxels)) * voxel
    out = dict(resolution=res, max_side=a.max_side, simplify_voxels=a.simplify_voxels, max_dist=reach, max_dist_voxels=reach / voxel,
               warmup=a.warmup, reps=a.reps, voxel=voxel)
    vol = lattice(res, syn.density)
    detail = mesh.marching_cubes(vol, syn.SIGMA_INSIDE / 2, (LO, HI))
    del vol
    target = mesh.simplify_clusters(detail, mesh._grid(a.simplify_voxels * voxel, None)[0], origin=LO).faces.shape[0]
    low = mesh.decimate(detail, unit, target_faces=target)
    v, f, extra = mesh._check_mesh(low)
    low = mesh.Mesh(v, f, extra[0] if extra[0] is not None else mesh.vertex_normals(low))
    out.update(detail_vertices=detail.vertices.shape[0], detail_faces=detail.faces.shape[0], vertices=v.shape[0], faces=f.shape[0])
    box = (LO, HI)
    size = mesh.fit_texel_size(low, a.max_side)
    t = mesh.texture_atlas(low, texel_size=size)
    low.texture = t
    n = t.width * t.height
    out["atlas"] = dict(width=t.width, height=t.height, texel_size=size, texel_size_voxels=size / voxel)
    points, dirs, valid = mesh.texel_points(low, t, box)
    own = -dirs

    dv, df, dvn = mesh._detail(detail)
    times = {}
    times["grid_build_ms"] = wall_ms(lambda: mesh._normal_grid(dv, df, reach), a.warmup, a.reps)
    grid = mesh._normal_grid(dv, df, reach)
    out["grid"] = dict(cell=grid.cell, cell_voxels=grid.cell / voxel, dims=list(grid.dims), entries=grid.n_entries)
    keep = valid != 0                                            # the same queries for both kernels: the valid texels, in atlas order
    vp, vm = points[keep].contiguous(), own[keep].contiguous()
    times["transfer_normals_ms"] = wall_ms(lambda: mesh.transfer_normals(vp, vm, detail, reach, grid=grid), a.warmup, a.reps)
    times["transfer_normals_two_sided_ms"] = wall_ms(lambda: mesh.transfer_normals(vp, vm, detail, reach, oriented=False, grid=grid), a.warmup, a.reps)
    times["closest_on_mesh_ms"] = wall_ms(lambda: mesh.closest_on_mesh(vp, detail, max_dist=reach, return_points=True, grid=grid), a.warmup, a.reps)
    del vp, vm
    nrm, dist, face, _, dbg = mesh.transfer_normals(points, own, detail, reach, grid=grid, valid=valid, return_debug=True)
    live = valid != 0
    hit = live & (face >= 0)
    out.update(texels=n, valid_texels=int(live.sum()), hit_texels=int(hit.sum()), hit_share=float(hit.sum()) / max(int(live.sum()), 1),
               mean_shells=float(dbg[live, 0].float().mean()), mean_faces_evaluated=float(dbg[live, 1].float().mean()),
               max_faces_evaluated=int(dbg[:, 1].max()), mean_distance_voxels=float(dist[hit].mean()) / voxel)
    two_sided_face = mesh.transfer_normals(points, own, detail, reach, oriented=False, grid=grid, valid=valid)[2]
    out["winners_changed_by_orientation"] = int((two_sided_face[live] != face[live]).sum())
    del dbg, dist, two_sided_face

    times["bake_normal_map_ms"] = wall_ms(lambda: mesh.bake_normal_map(low, detail, reach, box=box), a.warmup, a.reps)
    from ngp_pl_amd.networks import NGP
    model = NGP(scale=0.5).cuda()
    times["bake_texture_ms"] = wall_ms(lambda: mesh.bake_texture(model, low, texel_size=size), a.warmup, a.reps)
    out["times"] = {k: dict(median=x[0], min=x[1], max=x[2]) for k, x in times.items()}

    # quality against the scene's own surface
    nm = mesh.bake_normal_map(low, detail, reach, box=box)
    decoded = nm.image.view(-1, 3).double() * (2.0 / 255.0) - 1.0
    truth = true_normals(points, 0.25 * voxel)
    flat = torch.zeros(n, 3, dtype=torch.float64, device=points.device)
    # the face of a texel: the nearest face of the simplified mesh itself (the texel lies on it)
    own_face = mesh.closest_on_mesh(points, mesh.Mesh(v, f), max_dist=reach)[1].long()
    ok = live & (own_face >= 0)
    tri = v[f[own_face.clamp(min=0)].long()].double()
    flat[ok] = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])[ok]
    out["angular_error_deg"] = dict(normal_map=angle_stats(decoded, truth, hit & ok), vertex_normals=angle_stats(own, truth, hit & ok),
                                    face_normals=angle_stats(flat, truth, hit & ok))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
