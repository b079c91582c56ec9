"""Times of the mesh-distance stages (libngp_meshdist.so) on the procedural scene: the marching-cubes mesh of the scene's true
density at `--resolution`^3 (threshold SIGMA_INSIDE / 2) against its simplification with cells of `--simplify-voxels` (2) voxels,
in both directions: sample_surface, the grid build, the query and the statistics, each wall time with a device sync, two warm-up
calls, the median of `--reps` (7); beside them the marching cubes and the simplification of the same run, the shells visited and
the faces evaluated per query, and the numpy brute force (tests/mesh_distance_reference.py) at the largest number of point x face
pairs it finishes within `--brute-seconds`.  Then the accuracy of the export against the level-0 marching-cubes mesh of the
scene's signed distance on the same lattice: Chamfer, Hausdorff and F-score at one and at a quarter of a lattice step.  Prints
one JSON line.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ngp_pl_amd import mesh, synthetic as syn
from tests import mesh_distance_reference as R

LO, HI = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)


def timed(fn, reps):
    """(median, min, max) wall seconds of fn with a device sync, after two warm-up calls, and fn's last result."""
    for _ in range(2):
        out = fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return (statistics.median(times), min(times), max(times)), out


def lattice(res, fn, chunk=1 << 24):
    """fn at every lattice point of the unit box, (res, res, res) f32, in chunks."""
    vol = torch.empty(res ** 3, dtype=torch.float32, device="cuda")
    for begin in range(0, res ** 3, chunk):
        n = min(chunk, res ** 3 - begin)
        vol[begin:begin + n] = fn(mesh.lattice_points((res,) * 3, (LO, HI), begin=begin, count=n))
    return vol.view(res, res, res)


def direction(src, dst, spacing, reps):
    """The four stages for the samples of src against dst."""
    v, f, _ = mesh._check_mesh(dst)
    row = {}
    row["sample_surface_s"], (p, w, _) = timed(lambda: mesh.sample_surface(src, spacing), reps)
    row["grid_build_s"], grid = timed(lambda: mesh.distance_grid(dst), reps)
    row["query_s"], (d2, face, _, dbg) = timed(lambda: mesh._query(p, v, f, grid, None, False, True), reps)
    row["query_without_counters_s"], _ = timed(lambda: mesh._query(p, v, f, grid, None, False, False), reps)
    row["statistics_s"], st = timed(lambda: mesh._stats(d2, face, w, []), reps)
    dbg = dbg.double()
    row.update(samples=p.shape[0], target_faces=f.shape[0], grid_dims=grid.dims, grid_cell=grid.cell, grid_entries=grid.n_entries,
               shells_per_query=dbg[:, 0].mean().item(), faces_evaluated_per_query=dbg[:, 1].mean().item(),
               faces_evaluated_max=dbg[:, 1].max().item(), mean=(st[1] / st[0]).item(), max=st[3].item())
    return row


def brute_force(src, dst, spacing, seconds):
    """The numpy brute force on the first n samples x all faces, n doubled until a run would pass `seconds`."""
    p = mesh.sample_surface(src, spacing)[0].cpu().numpy()
    v, f = dst.vertices.cpu().numpy(), dst.faces.cpu().numpy()
    n, took, done = 16, 0.0, None
    while n <= len(p):
        t0 = time.perf_counter()
        R.query_f32(p[:n], v, f, chunk=max(1, (1 << 22) // max(len(f), 1)))
        took = time.perf_counter() - t0
        done = dict(points=n, faces=len(f), pairs=n * len(f), seconds=took)
        if took * 2 > seconds:
            break
        n *= 2
    return done


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--simplify-voxels", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--brute-seconds", type=float, default=60.0, help="0 skips the numpy brute force")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "meshdist_bench needs a GPU"
    res, voxel = a.resolution, 1.0 / (a.resolution - 1)
    out = dict(resolution=res, simplify_voxels=a.simplify_voxels, reps=a.reps)
    vol = lattice(res, syn.density)
    out["marching_cubes_s"], export = timed(lambda: mesh.marching_cubes(vol, syn.SIGMA_INSIDE / 2, (LO, HI)), a.reps)
    del vol
    export = mesh.Mesh(export.vertices, export.faces)
    out["simplify_s"], slim = timed(lambda: mesh.simplify_clusters(export, a.simplify_voxels * voxel, origin=LO), a.reps)
    out.update(export_vertices=export.vertices.shape[0], export_faces=export.faces.shape[0], simplified_vertices=slim.vertices.shape[0],
               simplified_faces=slim.faces.shape[0], spacing=voxel)
    out["export_to_simplified"] = direction(export, slim, voxel, a.reps)
    out["simplified_to_export"] = direction(slim, export, voxel, a.reps)
    out["mesh_distance_s"], r = timed(lambda: mesh.mesh_distance(export, slim, spacing=voxel, thresholds=(voxel, voxel / 4)), a.reps)
    out["export_vs_simplified"] = r
    if a.brute_seconds > 0:
        out["numpy_brute_force"] = brute_force(export, slim, voxel, a.brute_seconds)
    sd = lattice(res, lambda x: -syn.signed_distance(x))
    truth = mesh.marching_cubes(sd, 0.0, (LO, HI))
    del sd
    out["export_vs_truth"] = mesh.mesh_distance(export, mesh.Mesh(truth.vertices, truth.faces), spacing=voxel, thresholds=(voxel, voxel / 4))
    out["lattice_diagonal"] = 3 ** 0.5 * voxel
    print(json.dumps(out))


if __name__ == "__main__":
    main()
