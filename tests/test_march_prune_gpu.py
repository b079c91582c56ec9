"""GPU: the native stepper's pruned train march (csrc/march.hip: march_reach_table_kernel, march_reach_far) changes no bit.
(a) marches with the pruning on and off, and the API-shaped march, on the same bitfields; (b) 40 trainer steps across two occupancy
updates with the pruning on and off; (c) a configuration the pruning does not apply to (scale 16: six cascades, exponential steps)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from ngp_pl_amd import synthetic as syn

pytestmark = pytest.mark.gpu

G = 128
N_RAYS = 2048


def _rays(n, seed):
    g = np.random.RandomState(seed)
    W = 200
    dirs = syn.get_ray_directions(W, W, syn.intrinsics(W))
    poses = syn.hemisphere_poses(16, seed=1)
    ro, rd = syn.get_rays(dirs[torch.from_numpy(g.randint(0, W * W, n))], poses[torch.from_numpy(g.randint(0, 16, n))])
    return ro.cuda().contiguous(), rd.cuda().contiguous()


def _cells(cells):
    grid = np.zeros((1, G ** 3), np.float32)
    if len(cells):
        grid[0, syn.morton3D_np(np.asarray(cells))] = 1.0
    return syn.pack_bitfield_np(grid, 0.5)


BITFIELDS = {
    "empty": lambda: _cells(np.zeros((0, 3), np.int64)),
    "full": lambda: np.full(G ** 3 // 8, 255, np.uint8),
    "one_cell": lambda: _cells([[64, 64, 64]]),
    "pillar": lambda: _cells([[64, 71, z] for z in range(G)]),                                # one cell thick, on a block face
    "border_cells": lambda: _cells([[127, 60, 0], [0, 0, 0], [5, 127, 127]]),
    "blob": lambda: syn.random_blob_bitfield(1, G, 0.08, seed=1),
    "scene": lambda: syn.pack_bitfield_np(syn.analytic_density_grid(1, 0.5, G), 5.0),         # the procedural object: what late training marches
}


class _Stepper:
    """A Trainer's native stepper, created with NGP_MARCH_PRUNE as given (the library reads it when a stepper is created)."""

    def __init__(self, prune, scale=0.5):
        from ngp_pl_amd.networks import NGP
        from ngp_pl_amd.trainer import Trainer
        torch.manual_seed(0)
        self.model = NGP(scale=scale).cuda()
        self.model.register_training_buffers()
        self.tr = Trainer(self.model)
        old = os.environ.get("NGP_MARCH_PRUNE")
        os.environ["NGP_MARCH_PRUNE"] = "1" if prune else "0"
        try:
            self.B = self.tr.buffers(N_RAYS)
            self.h = self.tr._native_stepper(self.B)
        finally:
            if old is None:
                del os.environ["NGP_MARCH_PRUNE"]
            else:
                os.environ["NGP_MARCH_PRUNE"] = old

    def march(self, bitfield, ro, rd):
        """One march of the stepper on its marching stream; every output as host arrays."""
        from ngp_pl_amd._lib import call, stream
        self.model.density_bitfield.copy_(torch.from_numpy(bitfield).cuda().view_as(self.model.density_bitfield))
        torch.cuda.synchronize()
        B = self.B
        call("ngp_stepper_march", self.h, ro.data_ptr(), rd.data_ptr(), stream(), self.tr.side.cuda_stream)
        call("ngp_stepper_drop_pending", self.h)             # waits for the march and hands record set 0 back
        torch.cuda.synchronize()
        S = int(B.counter_np[0][0])
        assert 0 <= S <= B.cap and int(B.counter_np[0][1]) == N_RAYS
        v = B.sample_views(S, 0)
        out = dict(hits=B.view("hits_t0", torch.float32, N_RAYS, 2), noise=B.noise[0], rays_a=B.view("rays_a0", torch.int64, N_RAYS, 3),
                   xyzs=v["xyzs"], dirs=v["dirs"], deltas=v["deltas"], ts=v["ts"])
        out = {k: t.cpu().numpy().copy() for k, t in out.items()}
        out["S"] = S
        return out


def _guards(reset):
    from ngp_pl_amd._lib import call
    g = (C.c_uint32 * 4)()
    call("ngp_march_guard_read", g, 1 if reset else 0)
    return list(g)


def _same(a, b, what):
    assert a["S"] == b["S"], (what, a["S"], b["S"])
    for k in ("hits", "noise", "rays_a", "xyzs", "dirs", "deltas", "ts"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), "%s: %s differs" % (what, k)


def _api_march(model, esf, ro, rd, hits, noise):
    """The API-shaped march (ngp_raymarching_train_count / _write, which never prune) on the stepper's own hits and jitter."""
    import ngp_pl_amd.vren as vren
    rays_a, xyzs, dirs, deltas, ts, counter = vren.raymarching_train(ro, rd, torch.from_numpy(hits).cuda(), model.density_bitfield, model.cascades,
                                                                     float(model.scale), esf, torch.from_numpy(noise).cuda(), model.grid_size, 1024)
    S = int(counter[0].item())
    return dict(S=S, rays_a=rays_a.cpu().numpy(), xyzs=xyzs[:S].cpu().numpy(), dirs=dirs[:S].cpu().numpy(), deltas=deltas[:S].cpu().numpy(),
                ts=ts[:S].cpu().numpy())


@pytest.fixture(scope="module")
def steppers():
    return _Stepper(True), _Stepper(False)


@pytest.mark.parametrize("name", list(BITFIELDS))
def test_marches_with_and_without_pruning_are_the_same_bits(steppers, name):
    on, off = steppers
    bf = BITFIELDS[name]()
    ro, rd = _rays(N_RAYS, seed=7)
    _guards(True)
    a, b = on.march(bf, ro, rd), off.march(bf, ro, rd)
    assert _guards(False)[:3] == [0, 0, 0]
    _same(a, b, name)
    counts = a["rays_a"][:, 2]
    assert np.array_equal(a["rays_a"][:, 0], np.arange(N_RAYS)) and counts.sum() == a["S"]
    assert np.array_equal(a["rays_a"][:, 1], np.cumsum(counts) - counts)
    print("%s: S = %d, rays with samples %d of %d" % (name, a["S"], (counts > 0).sum(), N_RAYS))
    if name == "empty":
        assert a["S"] == 0
    if name in ("full", "scene", "blob"):               # (a single 1/128 cell may be missed by all 2048 rays)
        assert a["S"] > 0
    # ... and the march of the API-shaped entry points, which this change leaves alone
    api = _api_march(on.model, 0.0, ro, rd, a["hits"], a["noise"])
    assert api["S"] == a["S"]
    for k in ("rays_a", "xyzs", "dirs", "deltas", "ts"):
        assert np.array_equal(api[k].view(np.uint8), a[k].view(np.uint8)), "%s: %s differs from the API-shaped march" % (name, k)


def _train(prune, steps=40, n=1024):
    from ngp_pl_amd.bench_support import GpuDataset
    from ngp_pl_amd.networks import NGP
    from ngp_pl_amd.trainer import Trainer
    old = os.environ.get("NGP_MARCH_PRUNE")
    os.environ["NGP_MARCH_PRUNE"] = "1" if prune else "0"
    try:
        dev = torch.device("cuda")
        torch.manual_seed(3)
        m = NGP(scale=0.5).cuda()
        m.register_training_buffers()
        tr = Trainer(m, warmup_steps=16)                  # the second update (step 16) already thresholds the grid: sparse from there on
        data = GpuDataset(64, 8, dev, seed=0)
        gen = torch.Generator(device=dev).manual_seed(11)
        batches = [data.sample(n, gen) for _ in range(steps + 1)]
        per_ray = []
        for it in range(steps):
            ro, rd, gt = batches[it]
            last = tr.step(ro, rd, gt, next_batch=batches[it + 1][:2])
            per_ray.append([last["rgb"].clone(), last["opacity"].clone(), last["total"].clone(), torch.tensor([last["rm_samples"]])])
        torch.cuda.synchronize()
        assert tr.global_step == steps > 2 * tr.update_interval
        state = dict(enc=m.xyz_encoder.params.detach().clone(), rgb=m.rgb_net.params.detach().clone(), grid=m.density_grid.clone(),
                     bits=m.density_bitfield.clone())
        return state, per_ray
    finally:
        if old is None:
            del os.environ["NGP_MARCH_PRUNE"]
        else:
            os.environ["NGP_MARCH_PRUNE"] = old


def test_trainer_steps_with_and_without_pruning_are_the_same_bits():
    _guards(True)
    (sa, pa), (sb, pb) = _train(True), _train(False)
    assert _guards(False)[:3] == [0, 0, 0]
    for k in sa:
        assert torch.equal(sa[k].view(torch.uint8), sb[k].view(torch.uint8)), "parameters differ: %s" % k
    for it, (x, y) in enumerate(zip(pa, pb)):
        for u, w in zip(x, y):
            assert torch.equal(u.view(torch.uint8), w.view(torch.uint8)), "per-ray outputs differ at step %d" % it
    occ = (sa["bits"].cpu().numpy().reshape(-1)[:, None] >> np.arange(8) & 1).mean()
    rm = [int(x[3]) for x in pa]
    print("occupied share after 40 steps %.3f, samples per step first %d last %d" % (occ, rm[0], rm[-1]))
    assert 0.0 < occ < 1.0 and rm[-1] > 0                   # a grid the pre-test has something to decide on


def test_a_cascaded_configuration_marches_as_before():
    """Scale 16 (six cascades, exp_step_factor 1/256): no reach table is built and the count kernel runs unchanged."""
    on, off = _Stepper(True, scale=16.0), _Stepper(False, scale=16.0)
    assert on.model.cascades > 1 and on.tr.exp_step_factor > 0
    bf = syn.random_blob_bitfield(on.model.cascades, G, 0.08, seed=2)
    ro, rd = _rays(N_RAYS, seed=9)
    _guards(True)
    a, b = on.march(bf, ro, rd), off.march(bf, ro, rd)
    assert _guards(False)[:3] == [0, 0, 0]
    _same(a, b, "scale 16")
    assert a["S"] > 0
    api = _api_march(on.model, on.tr.exp_step_factor, ro, rd, a["hits"], a["noise"])
    assert api["S"] == a["S"]
    for k in ("rays_a", "xyzs", "dirs", "deltas", "ts"):
        assert np.array_equal(api[k].view(np.uint8), a[k].view(np.uint8)), "scale 16: %s differs from the API-shaped march" % k
