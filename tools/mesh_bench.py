"""Mesh export timing on the trained procedural scene: trains `--steps` native steps, then times extract_mesh at `--resolution`
(wall time with a device sync, split into density volume and marching cubes; best of `--reps`) and prints one JSON line with V, F
and the marching cubes' algorithmic bytes (volume read twice + outputs).  Under `rocprofv3 --kernel-trace --stats` the kernel
times of the same extraction divide those bytes (rate / 8 TB/s = share of HBM peak)."""
import argparse
import json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--resolution", type=int, default=512)
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
    print(json.dumps(res))


if __name__ == "__main__":
    main()
