"""Times and figures of the quadric placement (libngp_meshquadric.so) on the procedural scene: the marching-cubes mesh of the
scene's true density at `--resolution`^3 (threshold SIGMA_INSIDE / 2), clustered with cells of `--simplify-voxels` (2) voxels.
Times: ngp_meshquadric_accumulate and ngp_meshquadric_place beside the simplifier's own three calls (cluster, count, emit) in the
same run, each call alone between two HIP events on preallocated buffers, after `--warmup` (3) calls, the median of `--reps` (15)
with min and max.  Figures: mesh_distance of the simplified mesh against the unsimplified one for placement "mean" and "quadric"
(Chamfer, Hausdorff, F-score at one and at half a voxel), the same against the level-0 marching-cubes mesh of the scene's signed
distance, and the share of the clusters in each state.  Prints one JSON line.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ngp_pl_amd import _meshquadric_lib as ql, _meshsimplify_lib as sl, mesh, synthetic as syn
from ngp_pl_amd._lib import ptr, stream

LO, HI = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)


def lattice(res, fn, chunk=1 << 24):
    """fn at every lattice point of the unit box, (res, res, res) f32, in chunks."""
    vol = torch.empty(res ** 3, dtype=torch.float32, device="cuda")
    for begin in range(0, res ** 3, chunk):
        n = min(chunk, res ** 3 - begin)
        vol[begin:begin + n] = fn(mesh.lattice_points((res,) * 3, (LO, HI), begin=begin, count=n))
    return vol.view(res, res, res)


def event_ms(fn, warmup, reps):
    """(median, min, max) milliseconds of fn between two events on the current stream."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def stage_times(v, f, normals, cell, warmup, reps):
    """The five calls on one set of buffers, in the order the wrapper issues them."""
    n_v, n_f, dev = v.shape[0], f.shape[0], v.device
    o = torch.tensor(LO, dtype=torch.float32, device=dev)
    label = torch.empty(n_v, dtype=torch.int32, device=dev)
    sws_bytes = sl.lib().ngp_meshsimplify_workspace_bytes(n_v, n_f)
    qws_bytes = ql.lib().ngp_meshquadric_workspace_bytes(n_v, n_f)
    sws = torch.empty(sws_bytes, dtype=torch.uint8, device=dev)
    qws = torch.empty(qws_bytes, dtype=torch.uint8, device=dev)
    totals = torch.empty(3, dtype=torch.int64, device=dev)
    qtotals = torch.empty(3, dtype=torch.int64, device=dev)
    positions = torch.zeros(n_v, 3, dtype=torch.float32, device=dev)
    state = torch.empty(n_v, dtype=torch.uint8, device=dev)
    s = stream()

    def cluster():
        sl.call("ngp_meshsimplify_cluster", ptr(v), ptr(normals), None, n_v, ptr(o), cell, ptr(sws), sws_bytes, ptr(label), s)

    def count():
        sl.call("ngp_meshsimplify_count", ptr(f), ptr(label), n_v, n_f, ptr(sws), sws_bytes, ptr(totals), s)

    out = {}
    out["simplify_cluster_ms"] = event_ms(cluster, warmup, reps)
    out["simplify_count_ms"] = event_ms(count, warmup, reps)
    n_ov, n_of, n_clusters = totals.tolist()
    vo, no = torch.empty(n_ov, 3, device=dev), torch.empty(n_ov, 3, device=dev)
    fo = torch.empty(n_of, 3, dtype=torch.int32, device=dev)

    def emit():
        sl.call("ngp_meshsimplify_emit", ptr(v), n_v, n_f, ptr(o), cell, ptr(sws), sws_bytes, n_ov, n_of, ptr(vo), ptr(no), None, ptr(fo), s)

    def accumulate():
        ql.call("ngp_meshquadric_accumulate", ptr(v), ptr(f), ptr(label), n_v, n_f, ptr(o), cell, ptr(qws), qws_bytes, s)

    def place():
        ql.call("ngp_meshquadric_place", ptr(v), ptr(label), n_v, ptr(o), cell, ptr(qws), qws_bytes, ptr(positions), ptr(state), ptr(qtotals), s)

    out["simplify_emit_ms"] = event_ms(emit, warmup, reps)
    out["quadric_accumulate_ms"] = event_ms(accumulate, warmup, reps)
    out["quadric_place_ms"] = event_ms(place, warmup, reps)
    q, no_faces, outside = qtotals.tolist()
    out.update(clusters=n_clusters, output_vertices=n_ov, output_faces=n_of, quadric=q, mean_no_faces=no_faces, mean_outside=outside,
               mean_outside_share=outside / max(n_clusters, 1), corners_per_cluster=3.0 * n_f / max(n_clusters, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--simplify-voxels", type=float, default=2.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "meshquadric_bench needs a GPU"
    res, voxel = a.resolution, 1.0 / (a.resolution - 1)
    cell = a.simplify_voxels * voxel
    out = dict(resolution=res, simplify_voxels=a.simplify_voxels, warmup=a.warmup, reps=a.reps, voxel=voxel)
    vol = lattice(res, syn.density)
    export = mesh.marching_cubes(vol, syn.SIGMA_INSIDE / 2, (LO, HI))
    del vol
    v, f, extra = mesh._check_mesh(export)
    out.update(export_vertices=v.shape[0], export_faces=f.shape[0])
    out["times"] = stage_times(v, f, extra[0], mesh._grid(cell, None)[0], a.warmup, a.reps)
    sd = lattice(res, lambda x: -syn.signed_distance(x))
    truth = mesh.marching_cubes(sd, 0.0, (LO, HI))
    del sd
    truth = mesh.Mesh(truth.vertices, truth.faces)
    full = mesh.Mesh(export.vertices, export.faces)
    slim = {}
    for placement in mesh.PLACEMENTS:
        m = mesh.simplify_clusters(export, cell, origin=LO, placement=placement)
        slim[placement] = m = mesh.Mesh(m.vertices, m.faces)
        out[placement + "_vs_export"] = mesh.mesh_distance(m, full, spacing=voxel, thresholds=(voxel, voxel / 2))
        out[placement + "_vs_truth"] = mesh.mesh_distance(m, truth, spacing=voxel, thresholds=(voxel, voxel / 2))
    out["export_vs_truth"] = mesh.mesh_distance(full, truth, spacing=voxel, thresholds=(voxel, voxel / 2))
    assert torch.equal(slim["mean"].faces, slim["quadric"].faces)
    moved = (slim["quadric"].vertices - slim["mean"].vertices).norm(dim=1)
    out["quadric_minus_mean_voxels"] = dict(mean=(moved.mean() / voxel).item(), max=(moved.max() / voxel).item())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
