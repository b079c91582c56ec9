"""Brick-sparse mesh extraction against the dense one on the trained procedural scene: trains `--steps` native steps (the scene and
the batches of tools/mesh_bench.py), then, at each of `--resolutions`, runs extract_mesh and extract_mesh(sparse=True) in turn,
`--reps` rounds after a warm-up round, and prints one JSON line per resolution with, for each of the two: the wall time with a
device sync (best and median of the rounds), the peak device memory of a round (torch's allocator, over what the model holds), V and
F; for the sparse path also its split into the mask from the bitfield, the brick index, the field evaluation and the marching cubes
(each with a sync), the bricks meshed and sampled, the share of lattice points sampled, and the faces of the dense mesh that the
sparse one does not have with their share (both meshes are in the dense numbering, so the sparse mesh's triangles are looked up
among the dense mesh's by their three positions).  `--sparse-only` lists resolutions at which only the sparse path runs.

Under `rocprofv3 --kernel-trace --stats` (a run of its own, `--reps 1`) the kernel times of the same extractions."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ngp_pl_amd import mesh
from ngp_pl_amd.networks import NGP
from ngp_pl_amd.trainer import Trainer
from tools.mesh_bench import batch


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base, out


def sparse_stages(model, n, threshold):
    """Wall time with a sync of each stage of the sparse path, and the SparseVolume's counts."""
    lo, hi = mesh._box(model)
    t_mask, _, mask = timed(lambda: mesh.brick_mask_from_occupancy(model, n))
    t_index, _, sv = timed(lambda: mesh.SparseVolume.index(n, mask))
    del sv
    t_volume, _, sv = timed(lambda: mesh.sparse_density_volume(model, n, mask=mask))
    t_mc, _, m = timed(lambda: mesh.marching_cubes_sparse(sv, threshold, (lo, hi)))
    return dict(mask_s=t_mask, index_s=t_index, index_and_density_s=t_volume, marching_cubes_sparse_s=t_mc, meshed_bricks=sv.n_mesh,
                sampled_bricks=sv.n_sample, bricks=mask.numel(), sampled_share=sv.sampled_share)


def missing_faces(dense, sparse):
    """Faces of `dense` whose three corner positions (bit patterns, in order) no face of `sparse` has."""
    def rows(m):
        r = m.vertices[m.faces.long()].reshape(-1, 9).view(torch.int32).long()
        key = torch.zeros(r.shape[0], dtype=torch.int64, device=r.device)
        for c in range(9):
            key = key * 1000003 + r[:, c]              # wraps: a hash, collisions only make `missing` smaller
        return key
    if dense.faces.shape[0] == 0:
        return 0
    return int((~torch.isin(rows(dense), rows(sparse))).sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--sparse-only", type=int, nargs="*", default=[2048], help="resolutions at which only the sparse path runs")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=20.0)
    a = ap.parse_args()
    torch.manual_seed(2)
    model = NGP(scale=0.5).cuda()
    model.register_training_buffers()
    tr = Trainer(model)
    bs = [batch(4096, 500 + i) for i in range(16)]
    for it in range(a.steps):
        tr.step(*bs[it % 16], next_batch=bs[(it + 1) % 16][:2])
    torch.cuda.synchronize()
    del tr, bs
    torch.cuda.empty_cache()
    for n in a.resolutions + a.sparse_only:
        both = n in a.resolutions
        times = dict(dense=[], sparse=[])
        peak = dict(dense=0, sparse=0)
        meshes = {}
        for _ in range(a.reps + 1):                   # the first round warms up (code objects, allocator); the two paths alternate
            for name in ("dense", "sparse") if both else ("sparse",):
                t, p, m = timed(lambda: mesh.extract_mesh(model, n, a.threshold, sparse=name == "sparse"))
                times[name].append(t)
                peak[name] = max(peak[name], p)
                meshes[name] = m
                del m
                torch.cuda.empty_cache()
        res = dict(resolution=n, steps=a.steps, reps=a.reps)
        for name, ts in times.items():
            if ts:
                res[name] = dict(best_s=min(ts[1:]), median_s=statistics.median(ts[1:]), rounds_s=ts[1:], peak_bytes=peak[name],
                                 V=meshes[name].vertices.shape[0], F=meshes[name].faces.shape[0])
        res["sparse"].update(sparse_stages(model, n, a.threshold))
        if both:
            F = meshes["dense"].faces.shape[0]
            missing = missing_faces(meshes["dense"], meshes["sparse"])
            res.update(dense_faces_missing_from_sparse=missing, missing_share=missing / F if F else 0.0,
                       sparse_faces_not_in_dense=missing_faces(meshes["sparse"], meshes["dense"]))
        meshes.clear()
        torch.cuda.empty_cache()
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
