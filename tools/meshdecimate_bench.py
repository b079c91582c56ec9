"""Times and figures of the edge-collapse decimation (libngp_meshdecimate.so) on the procedural scene of tools/meshquadric_bench.py:
the marching-cubes mesh of the scene's true density at `--resolution`^3 (threshold SIGMA_INSIDE / 2), decimated to the face count
that vertex clustering with cells of `--simplify-voxels` (2) voxels gives.
Times: the whole decimation `--reps` (5) times after `--warmup` (1): every ngp_meshdecimate_round and ngp_meshdecimate_apply between
two HIP events of its own (the host read of the round's totals lies between the two calls), their sums per run, and the wall time
of the loop with its host reads; the median run with min and max, and the median, min and max over the rounds of one run; beside
the simplifier's three calls (cluster, count, emit), each alone between two events, the median of 15 after 3.
Figures: mesh_distance (Chamfer, Hausdorff, F-score at one and at half a voxel) to the unsimplified mesh for the decimated mesh and
for simplify_clusters with "mean" and with "quadric" at the same face count.  Prints one JSON line.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ngp_pl_amd import _meshdecimate_lib as dl, _meshsimplify_lib as sl, mesh, synthetic as syn
from ngp_pl_amd._lib import ptr, stream
from tools.meshquadric_bench import HI, LO, event_ms, lattice


def spread(xs):
    return statistics.median(xs), min(xs), max(xs)


def decimate_once(v, f, cell, target, ws, ws_bytes, totals):
    """The loop of mesh._decimate on preallocated buffers, every call between events -> per-round (round ms, apply ms), the rounds'
    totals and the wall time in ms."""
    n_v, n_f = v.shape[0], f.shape[0]
    s = stream()
    events, rows, left = [], [], None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dl.call("ngp_meshdecimate_begin", ptr(f), n_v, n_f, ptr(ws), ws_bytes, s)
    while left is None or left > target:
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        dl.call("ngp_meshdecimate_round", ptr(v), n_v, n_f, cell, -1.0, ptr(ws), ws_bytes, ptr(totals), s)
        e[1].record()
        n_c, n_w, left = totals.tolist()
        if left <= target or n_c == 0:
            break
        keep = min(n_w, (left - target + 1) // 2)
        e[2].record()
        dl.call("ngp_meshdecimate_apply", n_v, n_f, n_w, keep, ptr(ws), ws_bytes, s)
        e[3].record()
        events.append(e)
        rows.append([n_c, n_w, left, keep])
        left -= 2 * keep
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return [(e[0].elapsed_time(e[1]), e[2].elapsed_time(e[3])) for e in events], rows, wall


def simplifier_times(v, f, normals, cell, warmup=3, reps=15):
    n_v, n_f, dev = v.shape[0], f.shape[0], v.device
    o = torch.tensor(LO, dtype=torch.float32, device=dev)
    label = torch.empty(n_v, dtype=torch.int32, device=dev)
    ws_bytes = sl.lib().ngp_meshsimplify_workspace_bytes(n_v, n_f)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    totals = torch.empty(3, dtype=torch.int64, device=dev)
    s = stream()
    out = {}
    out["simplify_cluster_ms"] = event_ms(lambda: sl.call("ngp_meshsimplify_cluster", ptr(v), ptr(normals), None, n_v, ptr(o), cell, ptr(ws),
                                                          ws_bytes, ptr(label), s), warmup, reps)
    out["simplify_count_ms"] = event_ms(lambda: sl.call("ngp_meshsimplify_count", ptr(f), ptr(label), n_v, n_f, ptr(ws), ws_bytes, ptr(totals), s),
                                        warmup, reps)
    n_ov, n_of, _ = totals.tolist()
    vo, no = torch.empty(n_ov, 3, device=dev), torch.empty(n_ov, 3, device=dev)
    fo = torch.empty(n_of, 3, dtype=torch.int32, device=dev)
    out["simplify_emit_ms"] = event_ms(lambda: sl.call("ngp_meshsimplify_emit", ptr(v), n_v, n_f, ptr(o), cell, ptr(ws), ws_bytes, n_ov, n_of,
                                                       ptr(vo), ptr(no), None, ptr(fo), s), warmup, reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--simplify-voxels", type=float, default=2.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "meshdecimate_bench needs a GPU"
    res, voxel = a.resolution, 1.0 / (a.resolution - 1)
    cell = mesh._grid(a.simplify_voxels * voxel, None)[0]
    unit = mesh._grid(voxel, None)[0]
    out = dict(resolution=res, simplify_voxels=a.simplify_voxels, warmup=a.warmup, reps=a.reps, voxel=voxel)
    vol = lattice(res, syn.density)
    export = mesh.marching_cubes(vol, syn.SIGMA_INSIDE / 2, (LO, HI))
    del vol
    v, f, extra = mesh._check_mesh(export)
    full = mesh.Mesh(export.vertices, export.faces)
    out.update(export_vertices=v.shape[0], export_faces=f.shape[0])
    slim = {p: mesh.simplify_clusters(export, cell, origin=LO, placement=p) for p in mesh.PLACEMENTS}
    target = slim["mean"].faces.shape[0]
    out["target_faces"] = target
    out["simplifier"] = simplifier_times(v, f, extra[0], cell)
    ws_bytes = dl.lib().ngp_meshdecimate_workspace_bytes(v.shape[0], f.shape[0])
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=v.device)
    totals = torch.empty(3, dtype=torch.int64, device=v.device)
    runs = [decimate_once(v, f, unit, target, ws, ws_bytes, totals) for _ in range(a.warmup + a.reps)][a.warmup:]
    assert all(r[1] == runs[0][1] for r in runs)                               # the same rounds every time
    per_round, rows, _ = sorted(runs, key=lambda r: r[2])[len(runs) // 2]
    out["decimate"] = dict(
        workspace_bytes=ws_bytes, rounds=len(rows), first_round=rows[0], last_round=rows[-1],
        wall_ms=spread([r[2] for r in runs]),
        round_calls_ms=spread([sum(t[0] for t in r[0]) for r in runs]), apply_calls_ms=spread([sum(t[1] for t in r[0]) for r in runs]),
        one_round_ms=spread([t[0] for t in per_round]), one_apply_ms=spread([t[1] for t in per_round]),
        first_round_ms=per_round[0][0], last_round_ms=per_round[-1][0])
    dec, stats = mesh.decimate(export, unit, target_faces=target, return_stats=True)
    assert stats["totals"][:len(rows)].tolist() == rows
    out["decimate"].update(output_vertices=dec.vertices.shape[0], output_faces=dec.faces.shape[0], reached=stats["reached"])
    for name, m in (("decimate", dec), ("mean", slim["mean"]), ("quadric", slim["quadric"])):
        out[name + "_vs_export"] = mesh.mesh_distance(mesh.Mesh(m.vertices, m.faces), full, spacing=voxel, thresholds=(voxel, voxel / 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
