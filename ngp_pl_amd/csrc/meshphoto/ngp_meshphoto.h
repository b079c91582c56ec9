/*
 * ngp_meshphoto.h -- C ABI of libngp_meshphoto.so: the colour of surface points (the texels of a texture atlas, or any other
 * points with a viewing direction) blended from photographs with known cameras, on gfx950.  Every point is projected into every
 * camera, tested against the depth buffer of the mesh in that camera, and the photographs that see it are sampled bilinearly and
 * blended with a weight that falls with the viewing angle.
 *
 * A library of its own beside the other thirteen (include/ngp_hip.h, ngp_mesh.h, ngp_meshfilter.h, ngp_meshcull.h,
 * ngp_meshsimplify.h, ngp_meshtsdf.h, ngp_meshsmooth.h, ngp_meshtex.h, ngp_metrics.h, ngp_meshdist.h, ngp_meshquadric.h,
 * ngp_meshdecimate.h and csrc/meshatlas/ngp_meshatlas.h), with their conventions: raw DEVICE pointers, caller-allocated outputs,
 * the hipStream_t passed as void*, 0 on success, a positive hipError_t if a launch failed, a negative NGP_E* code for bad
 * arguments.  No entry point allocates or synchronises, and every argument is checked on the host before anything is launched.
 * This header needs none of the others and may be included before or after them.  It lies beside the library's sources, not
 * under include/.  No other library is changed or needed: the depth buffers are an input, in the layout ngp_meshcull_views
 * leaves in its workspace after a call whose cameras fit one chunk.
 *
 * Points: points (n, 3) f32 in world coordinates, dirs (n, 3) f32 (the direction a viewer looks along at the point: minus the
 * surface normal) and valid (n) u8, as ngp_meshtex_texel_points and ngp_meshatlas_texel_points write them.  Cameras: poses
 * (n_cams, 3, 4) f32 row-major camera-to-world [R | t], K (3, 3) f32 row-major, photographs of W x H pixels: the conventions of
 * include/ngp_meshcull.h.  images (n_cams, H, W, 3) u8, row 0 on top; zbuf (n_cams, H, W) u32, the bits of the f32 depth of the
 * nearest surface per pixel and the bits of +inf (0x7F800000) where there is none.
 *
 * THE RULE.  All arithmetic is IEEE binary32, one rounding per operation, in the order written, left to right, no fused
 * multiply-add; divisions and square roots are correctly rounded; floor() is the f32 floor; a comparison with a NaN fails.
 *
 *   Camera c, with R = poses[c][:, 0:3] and t = poses[c][:, 3]:
 *     m[r][k] = R[k][r]                                         (row r of R^T)
 *     s[r]    = -(m[r][0] * t[0] + m[r][1] * t[1] + m[r][2] * t[2])
 *     o       = t                                               (the camera centre)
 *   A point x = (x0, x1, x2) in camera c, exactly as in include/ngp_meshcull.h:
 *     p[r] = m[r][0] * x0 + m[r][1] * x1 + m[r][2] * x2 + s[r]
 *     ud = K[0][0] * p[0] + K[0][1] * p[1] + K[0][2] * p[2],  vd and d likewise from rows 1 and 2 of K
 *     u = ud / d,  v = vd / d
 *
 *   A point with valid == 0, a coordinate that is not finite or a direction component that is not finite is SKIPPED for every
 *   camera: its acc and views are left as they are.  For every other point the cameras are visited in ascending index.  The
 *   sample of camera c is ACCEPTED when all of the following hold, tested in this order:
 *     1. d >= near.
 *     2. u >= 0.5  and  u <= (float)W - 0.5  and  v >= 0.5  and  v <= (float)H - 0.5: the bilinear footprint lies inside the
 *        photograph, nothing is extrapolated at a border.
 *     3. e_k = o_k - x_k,  L = sqrt((e_0 * e_0 + e_1 * e_1) + e_2 * e_2),  L > 0, and with
 *          cs = -((dir_0 * e_0 + dir_1 * e_1) + dir_2 * e_2) / L
 *        cs >= min_cos.
 *     4. ic = (int)floor(u), jc = (int)floor(v).  For every pixel (i, j) with max(ic - guard, 0) <= i <= min(ic + guard, W - 1)
 *        and max(jc - guard, 0) <= j <= min(jc + guard, H - 1), with z = zbuf[c][j][i] as an f32:
 *          d <= z + bias  and  z <= d + bias.
 *        The test is two-sided: a nearer surface in the window is an occluder or its silhouette; a farther one, or the +inf of
 *        an empty pixel, means that the point sits at its own silhouette or off the mesh, where its footprint picks up
 *        background.
 *   No index is formed from a value that has not passed tests 1 and 2: a NaN or a wild pose reads nothing.
 *
 *   An accepted sample is read bilinearly, pixel i having its centre at u = i + 0.5:
 *     X = u - 0.5,  i0 = (int)floor(X),  fx = X - floor(X),  i1 = min(i0 + 1, W - 1)
 *     Y = v - 0.5,  j0 = (int)floor(Y),  fy = Y - floor(Y),  j1 = min(j0 + 1, H - 1)
 *   and per channel k, with t(i, j) = (float)images[c][j][i][k]:
 *     top = t(i0, j0) * (1 - fx) + t(i1, j0) * fx
 *     bot = t(i0, j1) * (1 - fx) + t(i1, j1) * fx
 *     col_k = top * (1 - fy) + bot * fy
 *   Its weight is w = cs, multiplied by cs another power - 1 times (w = w * cs).  Then
 *     acc_k = acc_k + w * col_k  (k = 0, 1, 2),   acc_3 = acc_3 + w,   views = views + 1.
 *
 *   Resolve.  seen = valid != 0  and  views >= min_views  and  acc_3 > 0.  Where seen, rgb_k = (acc_k / acc_3) / 255; elsewhere
 *   rgb_k = 0.
 *
 * The sums of a point are formed serially, in camera order, by the one thread that owns the point (no atomic), and acc and views
 * carry them from one call to the next: every output is bit-identical run to run, for any launch shape and for any split of the
 * points or of the cameras into chunks, as long as the chunks of cameras are given in ascending order.
 */
#ifndef NGP_MESHPHOTO_H
#define NGP_MESHPHOTO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef NGP_EINVAL
#define NGP_EINVAL   (-1)  /* bad argument (null pointer, negative size, size or parameter out of range, not finite) */
#endif
#ifndef NGP_ERANGE
#define NGP_ERANGE   (-5)  /* more than INT32_MAX points or cameras in one call */
#endif

#define NGP_MESHPHOTO_MAX_GUARD 4
#define NGP_MESHPHOTO_MAX_POWER 8

/* ABI version of this library (1). */
int ngp_meshphoto_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshphoto_build_arch(void);

/* acc (n, 4) f32 and views (n) i32 are READ AND WRITTEN: the accepted samples of the cameras 0 .. n_cams - 1 of this call are
 * added to them in ascending order (THE RULE).  The caller zeroes both before the first chunk of cameras and passes them on to
 * the next; acc is 16-byte aligned (a point's four sums move as one vector).  images and zbuf hold the n_cams cameras of this call.  near_distance is the rule's `near` (finite); bias >= 0 and
 * finite, in world units; guard in 0..4 pixels; 0 < min_cos <= 1; power in 1..8.  W and H run from 1 to 16384, n_cams >= 1.
 * With n == 0 nothing is launched and the pointers are not looked at. */
int ngp_meshphoto_accumulate(const float* points, const float* dirs, const uint8_t* valid, int64_t n, const float* K, const float* poses,
                             int64_t n_cams, int W, int H, const uint8_t* images, const uint32_t* zbuf, float near_distance, float bias,
                             int guard, float min_cos, int power, float* acc, int32_t* views, void* stream);

/* rgb (n, 3) f32 and seen (n) u8 from acc, views and valid (THE RULE, Resolve).  min_views >= 1.  With n == 0 nothing is launched
 * and the pointers are not looked at. */
int ngp_meshphoto_resolve(const float* acc, const int32_t* views, const uint8_t* valid, int64_t n, int32_t min_views, float* rgb,
                          uint8_t* seen, void* stream);

#ifdef __cplusplus
}
#endif

#endif
