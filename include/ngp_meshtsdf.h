/*
 * ngp_meshtsdf.h -- C ABI of libngp_meshtsdf.so: fusion of per-camera depth maps into a truncated signed distance (TSDF) volume on
 * the lattice of the mesh export, on gfx950.  Marching cubes (include/ngp_mesh.h) at level 0 of that volume is the surface the
 * depth maps agree on.
 *
 * A library of its own beside libngp_hip.so (include/ngp_hip.h), libngp_mesh.so (include/ngp_mesh.h), libngp_meshfilter.so
 * (include/ngp_meshfilter.h), libngp_meshcull.so (include/ngp_meshcull.h) and libngp_meshsimplify.so (include/ngp_meshsimplify.h),
 * with their conventions: raw DEVICE pointers, caller-allocated state and outputs, the hipStream_t passed as void*, 0 on success,
 * a positive hipError_t if a launch failed, a negative NGP_E* code for bad arguments.  No entry point allocates or synchronises,
 * and every argument is checked on the host before anything is launched.  This header needs none of the other five and may be
 * included before or after them.
 *
 * Lattice: (nx, ny, nz) points over bounds6, a HOST pointer to {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z}; volumes and state arrays are
 * (nz, ny, nx), x fastest, point (i, j, k) at linear index (k*ny + j)*nx + i: the conventions of include/ngp_mesh.h.  Cameras:
 * poses (n_cams, 3, 4) f32 row-major camera-to-world [R | t], K (3, 3) f32 row-major, images of W x H pixels: the conventions of
 * include/ngp_meshcull.h.  depth is (n_cams, H, W) f32: per pixel the camera-space z (the rule's d) of the surface the pixel sees.
 *
 * THE RULE.  Every expression below is IEEE binary32, evaluated in the order written, left to right, each operation rounded on
 * its own (no fused multiply-add), divisions correctly rounded; floor() is the f32 floor.
 *
 *   Lattice point (i, j, k), per axis a with n = (nx, ny, nz)[a] and index = (i, j, k)[a], exactly as ngp_mesh_lattice_points:
 *     h[a] = (hi[a] - lo[a]) / (float)(n - 1)
 *     x[a] = lo[a] + (float)index * h[a]
 *
 *   Per-point state, which persists across calls; cleared state is all zero bytes:
 *     acc    f32   the sum of the truncated distances
 *     seen   i32   the number of cameras that contributed a distance
 *     behind i32   the number of cameras that saw the point hidden
 *
 *   Camera c, with R = poses[c][:, 0:3] and t = poses[c][:, 3] (as THE RULE of ngp_meshcull.h):
 *     m[r][k] = R[k][r]                                         (row r of R^T)
 *     s[r]    = -(m[r][0] * t[0] + m[r][1] * t[1] + m[r][2] * t[2])
 *     p[r] = m[r][0] * x0 + m[r][1] * x1 + m[r][2] * x2 + s[r]
 *     ud = K[0][0] * p[0] + K[0][1] * p[1] + K[0][2] * p[2],  vd and d likewise from rows 1 and 2 of K
 *     u = ud / d,  v = vd / d
 *
 *   Integrate.  For the cameras c = 0 .. n_cams-1 of a call, IN ASCENDING c, at every lattice point:
 *     skip the camera unless  d >= near  and  0 <= u < W  and  0 <= v < H          (a NaN fails each comparison)
 *     D = depth[c][floor(v)][floor(u)];  skip the camera unless D > 0
 *         (NaN, 0 and negative depths are "no observation"; +inf passes and means the pixel's ray met nothing)
 *     sdf = D - d
 *     if sdf < -trunc:   behind = behind + 1                    (the point is hidden by more than the truncation distance)
 *     otherwise:         q = sdf / trunc;  acc = acc + (q < 1 ? q : 1);  seen = seen + 1
 *   A point exactly at sdf == -trunc contributes -1 and is not behind.
 *
 *   Finish.
 *     vol = -(acc / (float)seen)     where seen > 0
 *     vol = +1                       where seen == 0 and behind > 0     (only ever hidden: inside)
 *     vol = -1                       where seen == 0 and behind == 0    (nothing ever looked there: empty)
 *
 *   Surface.  {vol > 0} is the solid: ngp_mesh_count / ngp_mesh_emit with threshold 0 triangulate it unchanged, and the normals come
 *   out outward because vol falls outward, as a density does.
 *
 * One thread owns one lattice point, walks the cameras in order and adds sequentially: there are no atomics.  The state after the
 * cameras 0 .. C-1 is therefore the same whether they arrive in one call or in any split into consecutive chunks, and every output
 * is bit-identical run to run and for any launch shape.
 */
#ifndef NGP_MESHTSDF_H
#define NGP_MESHTSDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef NGP_EINVAL
#define NGP_EINVAL   (-1)  /* bad argument (null pointer, size out of range, truncation not finite or not > 0) */
#endif
#ifndef NGP_ERANGE
#define NGP_ERANGE   (-5)  /* more than INT32_MAX cameras: the per-point counts do not fit int32 */
#endif

/* ABI version of this library (1). */
int ngp_meshtsdf_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshtsdf_build_arch(void);

/* Bytes of the per-point state of an nx x ny x nz lattice: 12 per point, that is three arrays (acc f32, seen i32, behind i32) of
 * 4 * nx * ny * nz bytes each, which need not be adjacent.  0 if a size is out of range (each axis 2..65535, at most 2^36 points,
 * as ngp_mesh_workspace_bytes has it). */
size_t ngp_meshtsdf_state_bytes(int nx, int ny, int nz);

/* Integrate (THE RULE above) the n_cams cameras of poses / depth into the state, in ascending camera index.  K, poses, depth, acc,
 * seen and behind are device pointers; depth is (n_cams, H, W) f32 and is addressed with 64-bit offsets, as the lattice is.  The
 * state is read once and written once per call, however many cameras there are.  W and H run from 1 to 16384, n_cams >= 1 (above
 * INT32_MAX: NGP_ERANGE); near_distance is the rule's `near`; trunc must be finite and > 0. */
int ngp_meshtsdf_integrate(int nx, int ny, int nz, const float* bounds6, const float* K, const float* poses, const float* depth,
                           int64_t n_cams, int W, int H, float near_distance, float trunc, float* acc, int32_t* seen, int32_t* behind,
                           void* stream);

/* Finish (THE RULE above): vol (n_points) f32 from the state of n_points lattice points.  vol may be acc itself.  n_points runs
 * from 0 to 2^36; with n_points == 0 nothing is launched and nothing is written. */
int ngp_meshtsdf_finish(int64_t n_points, const float* acc, const int32_t* seen, const int32_t* behind, float* vol, void* stream);

#ifdef __cplusplus
}
#endif

#endif
