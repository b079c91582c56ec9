"""Plain numpy float32 restatement of libngp_meshtsdf.so (include/ngp_meshtsdf.h, THE RULE), expression for expression: every
product and sum below is one f32 operation in the header's order (no `@`, no fused multiply-add), divisions are numpy's correctly
rounded f32 divisions.  `lattice`, `integrate`, `finish`, `tsdf`; and the analytic sphere scene the CPU and GPU tests share.  The
projection is tests/mesh_visibility_reference.py's.  Test infrastructure only."""
import numpy as np

from tests import mesh_visibility_reference as VR

F = np.float32


def lattice(resolution, bounds):
    """(nx * ny * nz, 3) f32 lattice points in linear order (x fastest), as ngp_mesh_lattice_points computes them."""
    nx, ny, nz = resolution
    lo, hi = np.asarray(bounds[0], F), np.asarray(bounds[1], F)
    axes = []
    for a, n in enumerate((nx, ny, nz)):
        h = (hi[a] - lo[a]) / F(n - 1)
        axes.append(lo[a] + np.arange(n, dtype=F) * h)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([axes[0][i.reshape(-1)], axes[1][j.reshape(-1)], axes[2][k.reshape(-1)]], 1)


def clear(n):
    """Cleared state of n points: acc f32, seen i32, behind i32, all zero."""
    return np.zeros(n, F), np.zeros(n, np.int32), np.zeros(n, np.int32)


def integrate(points, K, poses, img_wh, depths, near, trunc, state):
    """The cameras of `poses` / `depths` (C, H, W) in ascending order into state = (acc, seen, behind), in place."""
    W, H = img_wh
    acc, seen, behind = state
    near, trunc = F(near), F(trunc)
    depths = np.asarray(depths, F)
    for pose, img in zip(np.asarray(poses, F), depths):
        u, v, d = VR.project(points, K, pose)
        with np.errstate(all="ignore"):
            inside = (d >= near) & (u >= 0) & (u < F(W)) & (v >= 0) & (v < F(H))
            i = np.where(inside, np.floor(u), 0).astype(np.int64)
            j = np.where(inside, np.floor(v), 0).astype(np.int64)
            D = img[j, i]
            ok = inside & (D > 0)
            sdf = D - d
            hidden = ok & (sdf < -trunc)
            add = ok & ~hidden
            q = sdf / trunc
            q = np.where(q < 1, q, F(1))
            acc[add] = acc[add] + q[add]
        seen += add
        behind += hidden
    return state


def finish(state):
    """vol (n,) f32."""
    acc, seen, behind = state
    with np.errstate(all="ignore"):
        mean = -(acc / seen.astype(F))
    return np.where(seen > 0, mean, np.where(behind > 0, F(1), F(-1))).astype(F)


def tsdf(resolution, bounds, K, poses, img_wh, depths, near, trunc):
    """-> acc, seen, behind (n,), vol (nz, ny, nx)."""
    nx, ny, nz = resolution
    state = integrate(lattice(resolution, bounds), K, poses, img_wh, depths, near, trunc, clear(nx * ny * nz))
    return state + (finish(state).reshape(nz, ny, nx),)


# ---- the shared scene -------------------------------------------------------------------------------------------------------

def sphere_depths(K, poses, img_wh, radius=0.3, centre=(0.0, 0.0, 0.0)):
    """(C, H, W) f32: camera-space z of the first hit of each pixel centre's ray with the sphere, +inf where it misses (float64
    geometry, rounded once)."""
    W, H = img_wh
    K = np.asarray(K, np.float64)
    j, i = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    dirs = np.stack([(i - K[0, 2]) / K[0, 0], (j - K[1, 2]) / K[1, 1], np.ones_like(i)], -1)     # z = 1: the ray parameter is d
    out = []
    for P in np.asarray(poses, np.float64):
        rd = dirs @ P[:3, :3].T
        oc = P[:3, 3] - np.asarray(centre, np.float64)
        a, b, c = (rd * rd).sum(-1), (rd * oc).sum(-1), oc @ oc - radius * radius
        disc = b * b - a * c
        with np.errstate(invalid="ignore"):
            t = (-b - np.sqrt(disc)) / a
        out.append(np.where((disc >= 0) & (t > 0), t, np.inf))
    return np.stack(out).astype(F)


SPHERE = dict(radius=0.3, resolution=(48, 48, 48), bounds=((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)), img_wh=(96, 96), near=0.05,
              trunc=4.0 / 47)


def sphere_scene():
    """The sphere of radius 0.3 at the origin seen by 14 cameras at distance 1.5 (6 axis directions, 8 cube diagonals) at 96 x 96,
    a 48^3 lattice over [-0.5, 0.5]^3, trunc = 4 voxels: K, poses, depths."""
    K = VR.intrinsics(130, 48, 48)
    poses = VR.ring_cameras(1.5, (0.0, 0.0, 0.0))
    return K, poses, sphere_depths(K, poses, SPHERE["img_wh"], SPHERE["radius"])
