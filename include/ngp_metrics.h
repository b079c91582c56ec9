/*
 * ngp_metrics.h -- C ABI of libngp_metrics.so: image metrics on gfx950, the squared error behind PSNR and the structural
 * similarity index (SSIM) with the 11-tap Gaussian window, per image of a batch, with an optional mask.
 *
 * A library of its own beside libngp_hip.so (include/ngp_hip.h) and the seven mesh libraries (include/ngp_mesh*.h), with their
 * conventions: raw DEVICE pointers, caller-allocated outputs and workspace, the hipStream_t passed as void*, 0 on success, a
 * positive hipError_t if a launch failed, a negative NGP_E* code for bad arguments.  No entry point allocates or synchronises,
 * and every argument is checked on the host before anything is launched.  This header needs none of the other eight and may be
 * included before or after them.
 *
 * Images: f32, n images of h x w pixels with c channels, 1 <= c <= 4.  layout NGP_METRICS_HWC: (n, h, w, c), element
 * ((i * h + y) * w + x) * c + k; layout NGP_METRICS_CHW: (n, c, h, w), element ((i * c + k) * h + y) * w + x.  All addressing
 * is 64-bit.  mask: u8 (n, h, w) or NULL; a pixel is selected when its byte is non-zero (NULL selects all).  The inputs are
 * taken to be finite; no index depends on a value, so a non-finite input cannot cause an access out of bounds, and nothing else
 * is promised for it.
 *
 * THE RULE.  f32 operations are IEEE binary32, one rounding each, in the order written, left to right, no fused multiply-add;
 * divisions are correctly rounded.  (double)x widens exactly.
 *
 *   Squared error.  Per element d = p - t, e = d * d in f32; image i gets sum_i = the sum of (double)e over its selected pixels
 *   and all c channels, and count_i = c * (number of selected pixels).
 *
 *   Window.  g[k] = exp(-((k - 5) / 1.5)^2 / 2) for k = 0 .. 10, divided by their sum, computed in f64 and rounded to f32 once:
 *   NGP_METRICS_WINDOW below.
 *
 *   Filter.  For a map m (one channel of one image, h x w), 11 <= h, w:
 *     row pass     X(y, x) = the value of:  a = g[0] * m(y, x);  a = a + g[k] * m(y, x + k)  for k = 1 .. 10
 *                  for 0 <= y < h, 0 <= x < w - 10;
 *     column pass  F(y, x) = the value of:  a = g[0] * X(y, x);  a = a + g[k] * X(y + k, x)  for k = 1 .. 10
 *                  for 0 <= y < h - 10, 0 <= x < w - 10.
 *   F is (h - 10) x (w - 10): the valid region.  F(y, x) belongs to the window centred on pixel (y + 5, x + 5).
 *   Five maps are filtered per channel: p, t, p * p, t * t and p * t, the products formed in f32 before the filter.
 *
 *   Index.  With mp, mt, pp, tt, pt the five filtered values at (y, x):
 *     spp = pp - mp * mp,  stt = tt - mt * mt,  spt = pt - mp * mt
 *     num = ((2 * mp) * mt + c1) * (2 * spt + c2)
 *     den = ((mp * mp + mt * mt) + c1) * ((spp + stt) + c2)
 *     s   = num / den
 *   c1 = (float)((0.01 * data_range) * (0.01 * data_range)) and c2 = (float)((0.03 * data_range) * (0.03 * data_range)),
 *   the products in f64 on the host.
 *
 *   Score.  Image i gets sum_i = the sum of (double)s over the c channels and over the windows (y, x) whose centre pixel
 *   (y + 5, x + 5) is selected, and count_i = c * (number of such windows).  The mean is sum_i / count_i; the caller divides.
 *   The optional map receives every s, (n, h - 10, w - 10, c) for NGP_METRICS_HWC and (n, c, h - 10, w - 10) for
 *   NGP_METRICS_CHW, whether its window is selected or not.
 *
 *   Order of the sums.  A workgroup adds its values in f64 in an order fixed by the launch geometry (a thread its own values in
 *   a fixed sequence, the threads of a wave through a fixed shuffle tree, the waves in index order) and stores one partial sum and
 *   count into the workspace.  A second kernel adds an image's partials: lane l of one wave adds the partials l, l + 64, ... in
 *   index order, and the same shuffle tree adds the lanes.  No atomics: sum and count are bit-identical run to run.  The order
 *   depends on n, c, h, w and the layout only, not on the mask, the values or the map pointer.
 */
#ifndef NGP_METRICS_H
#define NGP_METRICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef NGP_EINVAL
#define NGP_EINVAL   (-1)  /* bad argument (null pointer, negative size, size out of range, workspace too small, not finite) */
#endif
#ifndef NGP_ERANGE
#define NGP_ERANGE   (-5)  /* a size above the limits of the entry point */
#endif

#define NGP_METRICS_HWC 0  /* channel-last (n, h, w, c) */
#define NGP_METRICS_CHW 1  /* planar (n, c, h, w) */

#define NGP_METRICS_MAX_CHANNELS 4
#define NGP_METRICS_MAX_SIDE 16384     /* h and w */
#define NGP_METRICS_WINDOW_TAPS 11

/* THE RULE's window, g[0] .. g[10]: 0.0010283801, 0.0075987582, 0.036000773, 0.10936069, 0.21300554, 0.26601171, mirrored. */
#define NGP_METRICS_WINDOW \
    { 0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f, \
      0x1.b43c4p-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f }

/* The output tile of the SSIM kernel: a workgroup owns NGP_METRICS_TILE_W x NGP_METRICS_TILE_H windows of one image. */
#define NGP_METRICS_TILE_W 64
#define NGP_METRICS_TILE_H 12
/* The squared-error kernel: workgroups of NGP_METRICS_SQ_THREADS threads, at most NGP_METRICS_SQ_MAX_BLOCKS per image, each
 * striding its image's c * h * w elements by (workgroups of the image) * NGP_METRICS_SQ_THREADS. */
#define NGP_METRICS_SQ_THREADS 256
#define NGP_METRICS_SQ_MAX_BLOCKS 512

/* ABI version of this library (1). */
int ngp_metrics_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_metrics_build_arch(void);

/* *w = NGP_METRICS_TILE_W, *h = NGP_METRICS_TILE_H.  Host only.  NGP_EINVAL for a null pointer. */
int ngp_metrics_tile(int* w, int* h);

/* Bytes of workspace that ngp_metrics_sq_error and ngp_metrics_ssim need for n images of c channels and h x w pixels: 16 per
 * workgroup partial.  0 if n < 1, c is outside [1, 4], h or w is outside [1, 16384] or the partials would number more than
 * INT32_MAX.  (h or w under 11 serves ngp_metrics_sq_error alone.) */
size_t ngp_metrics_workspace_bytes(int64_t n, int c, int h, int w);

/* sum (n) f64 and count (n) i64 of THE RULE's squared error between pred and target, n >= 1 images of 1 <= c <= 4 channels and
 * h x w pixels, 1 <= h, w <= 16384, in `layout`; mask (n, h, w) u8 or NULL.  workspace: device, 8-byte aligned, at least
 * ngp_metrics_workspace_bytes(n, c, h, w).  NGP_EINVAL for a null pointer (mask excepted), n < 1, c outside [1, 4], h or w < 1,
 * an unknown layout, or a workspace that is too small or misaligned; NGP_ERANGE for h or w above 16384 or more than INT32_MAX
 * partials.  Nothing is launched then. */
int ngp_metrics_sq_error(const float* pred, const float* target, const uint8_t* mask, int64_t n, int c, int h, int w, int layout,
                         void* workspace, size_t workspace_bytes, double* sum, int64_t* count, void* stream);

/* sum (n) f64 and count (n) i64 of THE RULE's index s between pred and target, n >= 1 images of 1 <= c <= 4 channels and h x w
 * pixels, 11 <= h, w <= 16384, in `layout`; mask (n, h, w) u8 or NULL; map f32 or NULL (THE RULE, Score).  data_range > 0 and
 * finite.  workspace as above.  NGP_EINVAL for a null pointer (mask and map excepted), n < 1, c outside [1, 4], h or w < 11, an
 * unknown layout, a data_range that is not > 0 and finite, or a workspace that is too small or misaligned; NGP_ERANGE for h or
 * w above 16384 or more than INT32_MAX partials.  Nothing is launched then. */
int ngp_metrics_ssim(const float* pred, const float* target, const uint8_t* mask, int64_t n, int c, int h, int w, int layout,
                     double data_range, void* workspace, size_t workspace_bytes, double* sum, int64_t* count, float* map,
                     void* stream);

#ifdef __cplusplus
}
#endif

#endif
