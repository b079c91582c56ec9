"""numpy restatement of the pruned train march's two pieces (csrc/march.hip): the reach table built from the bitfield
(march_reach_table_kernel) and the per-ray pre-test (march_reach_far), in float32 with the kernel's own operations in the kernel's
order.  One cascade, exp_step_factor 0, a 128^3 grid: the configuration the native stepper prunes.

fmaf(a, b, c) is formed as the float64 product (exact for float32 factors) plus c, rounded to float64 and then to float32: the same
value as the fused operation except where that double rounding straddles a tie, which no property checked against it depends on."""
import numpy as np

from ngp_pl_amd.synthetic import morton3D_np

G, NB = 128, 16                  # cells and 8^3 blocks per axis
F = np.float32


def _fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def reach_tables(bitfield):
    """(any, reach), both indexed [bz, by, bx]: any = some cell of the 8^3 block is occupied (the 512 Morton-consecutive cells from
    512 morton(bx, by, bz)), reach = OR of `any` over the block's 27-neighbourhood clamped at the grid border."""
    bits = np.unpackbits(np.ascontiguousarray(bitfield, np.uint8).reshape(-1)[:G ** 3 // 8], bitorder="little")
    any_b = bits.reshape(NB ** 3, 512).any(1)                                                                       # Morton order
    c = np.stack(np.meshgrid(np.arange(NB), np.arange(NB), np.arange(NB), indexing="ij"), -1).reshape(-1, 3)      # (bx, by, bz)
    any3 = np.zeros((NB, NB, NB), bool)
    any3[c[:, 2], c[:, 1], c[:, 0]] = any_b[morton3D_np(c)]
    reach = np.zeros((NB, NB, NB), bool)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                n = np.clip(c + np.array([dx, dy, dz]), 0, NB - 1)
                reach[c[:, 2], c[:, 1], c[:, 0]] |= any_b[morton3D_np(n)]
    return any3, reach


def block_of(x, bound0_inv):
    """march_probe's normalisation at 16 per axis, clamped to 0..15."""
    v = F(0.5) * (x * F(bound0_inv) + F(1)) * F(16.0)
    with np.errstate(invalid="ignore"):
        v = np.fmax(F(0), np.where(np.isnan(v), F(15.0), np.minimum(v, F(15.0))))         # fmaxf(0, fminf(v, 15)): fminf drops a NaN
        return v.astype(np.int32)


def pretest(rays_o, rays_d, t1, t2, reach, bound0=0.5):
    """Per ray with a hit (t1 >= 0; the interval BEFORE the jitter): (rejected, t2_cut, tested).  rejected: no walk, no samples.
    t2_cut <= t2: the far end the walk runs with.  tested False: the ray is not pruned (more than 62 points, non-finite inputs, no hit)."""
    o, d = np.asarray(rays_o, np.float32), np.asarray(rays_d, np.float32)
    t1, t2 = np.asarray(t1, np.float32), np.asarray(t2, np.float32)
    bound0 = F(bound0)
    bound0_inv = F(1) / bound0
    with np.errstate(all="ignore"):
        len2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        step = (bound0 * F(0.0625)) / np.sqrt(len2)
        q = (t2 - t1) / step
        mag = np.abs(o[:, 0]) + np.abs(o[:, 1]) + np.abs(o[:, 2]) + np.abs(d[:, 0]) + np.abs(d[:, 1]) + np.abs(d[:, 2]) + t2
        tested = (t1 >= 0) & (step > 0) & (step < F(3.0e38)) & (q >= 0) & (q < F(61.0)) & (mag < F(3.0e38))
        need = np.where(tested, q, 0).astype(np.int32) + 2
        lane = np.arange(64, dtype=np.float32)[None, :]
        t = _fma(lane, step[:, None], t1[:, None])
        b = [block_of(_fma(t, d[:, k:k + 1], o[:, k:k + 1]), bound0_inv) for k in range(3)]
        hit = reach[b[2], b[1], b[0]] & (np.arange(64)[None, :] < need[:, None]) & tested[:, None]
        any_hit = hit.any(1)
        last = 63 - np.argmax(hit[:, ::-1], 1)
        cut = np.minimum(t2, _fma((last + 1).astype(np.float32), step, t1))
    rejected = tested & ~any_hit
    t2_cut = np.where(tested & any_hit, cut, t2).astype(np.float32)
    return rejected, t2_cut, tested
