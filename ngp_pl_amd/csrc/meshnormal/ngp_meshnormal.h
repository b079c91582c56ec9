/*
 * ngp_meshnormal.h -- C ABI of libngp_meshnormal.so: normals carried from a detailed mesh onto the points of a simplified one
 * (the texels of its texture atlas, or any other points that come with a normal of their own), and the shading of a rendered
 * frame by a rendered normal map, on gfx950.  For every query point the nearest face of the detail mesh AMONG THE FACES THAT FACE
 * THE SAME WAY AS THE QUERY is found -- exactly the brute-force minimum, through the uniform grid of libngp_meshdist.so -- and the
 * detail mesh's vertex normals are interpolated at the closest point.
 *
 * A library of its own beside the other fourteen (include/ngp_hip.h, ngp_mesh.h, ngp_meshfilter.h, ngp_meshcull.h,
 * ngp_meshsimplify.h, ngp_meshtsdf.h, ngp_meshsmooth.h, ngp_meshtex.h, ngp_metrics.h, ngp_meshdist.h, ngp_meshquadric.h,
 * ngp_meshdecimate.h, csrc/meshatlas/ngp_meshatlas.h and csrc/meshphoto/ngp_meshphoto.h), with their conventions: raw DEVICE
 * pointers, caller-allocated outputs, the hipStream_t passed as void*, 0 on success, a positive hipError_t if a launch failed, a
 * negative NGP_E* code for bad arguments.  No entry point allocates or synchronises, and every argument is checked on the host
 * before anything is launched.  `origin` is a HOST pointer and is read during the call.  This header needs none of the others and
 * may be included before or after them: what it uses of include/ngp_meshdist.h is restated here.  It lies beside the library's
 * sources, not under include/.  No other library is changed or needed: the grid is an input, in the layout
 * ngp_meshdist_grid_count and ngp_meshdist_grid_fill leave it in.
 *
 * Detail mesh: vertices (n_vertices, 3) f32, faces (n_faces, 3) i32, vertex_normals (n_vertices, 3) f32; each may be NULL with its
 * size 0 (a null pointer with a positive size is NGP_EINVAL).  A face is USABLE when its three indices are inside [0, n_vertices)
 * and its nine coordinates are finite (the definition of include/ngp_meshdist.h).
 * Queries: points (n, 3) f32, query_normals (n, 3) f32 (the query's own normal m; for a texel, minus the direction
 * ngp_meshtex_texel_points / ngp_meshatlas_texel_points write) and valid (n) u8.
 *
 * THE RULE.  Every f32 expression below is IEEE binary32, evaluated in the order written, left to right, each operation rounded
 * on its own (no fused multiply-add); divisions and square roots are correctly rounded; a comparison with a NaN fails.
 * dot(x, y) = (x.x * y.x + x.y * y.y) + x.z * y.z.  x - y, x + y and s * x of vectors act per component.
 *
 * 1. ELIGIBLE FACES.  A face (a, b, c) is eligible for a query with normal m when it is usable and, if oriented != 0,
 *      ab = b - a,  ac = c - a
 *      g = (ab.y * ac.z - ab.z * ac.y,  ab.z * ac.x - ab.x * ac.z,  ab.x * ac.y - ab.y * ac.x)      (rule 1 of ngp_meshdist.h spells n so)
 *      dot(g, m) > 0.
 *    A NaN anywhere, a face of zero area and m = 0 make the comparison fail: such a face is not eligible.  With oriented == 0
 *    every usable face is eligible and m is not looked at here.
 *
 * 2. POINT TO TRIANGLE (C. Ericson, Real-Time Collision Detection, 5.1.5; rule 2 of ngp_meshdist.h, with the barycentric pair
 *    (v, w) of the deciding case beside the closest point q).  The first case that holds decides:
 *      ab = b - a,  ac = c - a,  ap = p - a,  d1 = dot(ab, ap),  d2 = dot(ac, ap)
 *      vertex a:   d1 <= 0 and d2 <= 0                          q = a                                   (v, w) = (0, 0)
 *      bp = p - b,  d3 = dot(ab, bp),  d4 = dot(ac, bp)
 *      vertex b:   d3 >= 0 and d4 <= d3                         q = b                                   (v, w) = (1, 0)
 *      vc = d1 * d4 - d3 * d2
 *      edge ab:    vc <= 0 and d1 >= 0 and d3 <= 0              v = d1 / (d1 - d3),  q = a + v * ab      (v, w) = (v, 0)
 *      cp = p - c,  d5 = dot(ab, cp),  d6 = dot(ac, cp)
 *      vertex c:   d6 >= 0 and d5 <= d6                         q = c                                   (v, w) = (0, 1)
 *      vb = d5 * d2 - d1 * d6
 *      edge ac:    vb <= 0 and d2 >= 0 and d6 <= 0              w = d2 / (d2 - d6),  q = a + w * ac      (v, w) = (0, w)
 *      va = d3 * d6 - d5 * d4
 *      edge bc:    va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    w = (d4 - d3) / ((d4 - d3) + (d5 - d6)),  q = b + w * (c - b)
 *                                                                                                       (v, w) = (1 - w, w)
 *      interior:   denom = 1 / ((va + vb) + vc),  v = vb * denom,  w = vc * denom,
 *                  v = 0 if not (v >= 0),  v = 1 if v > 1,  w = 0 if not (w >= 0),  w = 1 - v if w > 1 - v,
 *                  q = (a + v * ab) + w * ac                                                            (v, w) = the clamped (v, w)
 *      e = p - q,  d2 = (e.x * e.x + e.y * e.y) + e.z * e.z            (the squared distance; not the d2 of the dot products)
 *
 * 3. THE QUERY.  The result is the minimum of the 64-bit key  bits(d2) << 32 | face  over the eligible faces whose d2 is finite:
 *    the nearest eligible face, and the smaller index where d2 is bit-equal.  It is a MISS, (d2, face) = (+inf, -1), if there is no
 *    such face or if the minimum d2 > max_dist * max_dist (one f32 product).  This is by definition the brute-force minimum over
 *    every face of the detail mesh: the grid below never changes a bit of it.
 *
 * 4. THE NORMAL.  With (v, w) of the winning face by rule 2 and Na, Nb, Nc the vertex normals of its corners:
 *      u = (1 - v) - w
 *      N = (u * Na + v * Nb) + w * Nc                                  (per component)
 *      L = sqrt(dot(N, N))
 *    The output is N / L (per component) when L > 0 and L is finite.  Otherwise, and on a miss, it is the FALLBACK:
 *      Lm = sqrt(dot(m, m));  m / Lm (per component) when Lm > 0 and Lm is finite, else (0, 0, 1).
 *    bary receives (v, w), and (0, 0) on a miss.
 *    A query with valid == 0, or with a coordinate of p that is not finite, writes normal (0, 0, 0), d2 = +inf, face = -1,
 *    bary = (0, 0) and debug = (0, 0), and looks at nothing else.
 *
 * 5. SHADING.  Per pixel of camera c with ids >= 0, s the sample of the normal-map image (three f32 in [0, 1]) and l = lights[c]:
 *      t = 2 * s - 1                                                   (per component: one product, one difference)
 *      L = sqrt(dot(t, t))
 *      k = 1                                                           if not (L > 0) or L is not finite
 *      k = ambient + (1 - ambient) * max(dot(t / L, l), 0)             otherwise; max(x, 0) = x if x > 0, else 0
 *      out = albedo * k                                                (per component)
 *    A pixel with ids < 0 copies albedo.
 *
 * THE GRID (an acceleration; it is not part of the rule) is the one ngp_meshdist_grid_count and ngp_meshdist_grid_fill build for
 * the detail mesh: nx x ny x nz cubic cells of edge `cell`, the first at `origin`, cell (x, y, z) with the index
 * (z * ny + y) * nx + x, the cell of a coordinate t on an axis with n cells and origin o
 *      g = floor((t - o) / cell);   0 if not (g >= 0),  n - 1 if g >= n,  else (int)g,
 * every usable face entered into the cells of its box padded by s_f = slack(max(M_grid, the largest |coordinate| of the face)),
 * slack(m) = NGP_MESHNORMAL_SLACK_ULPS * 2^-23 * m, M_grid the largest of |origin| and |origin + n * cell| over the axes.  The
 * workspace holds 8 bytes per block of NGP_MESHNORMAL_SCAN_BLOCK cells, then the start of every cell's list, (cells + 1) u32, then
 * 4 bytes per cell that this library does not read; the faces of cell c are entries[start[c] .. start[c + 1]).
 * A query visits the Chebyshev shells r = 0, 1, 2, ... of cells around its own (clamped) cell, evaluates rules 1 and 2 on every
 * face listed there, and stops after shell r on the three tests of ngp_meshdist.h: with rc = (float)r * cell and
 * s_q = slack(max(M_grid, the largest |coordinate| of p)),
 *      sqrt(best d2) + s_q <= rc,   or   rc - s_q > max_dist,   or   shell r + 1 holds no cell of the grid.
 * The filter of rule 1 only removes candidates.  The derivation (a)-(f) of ngp_meshdist.h bounds the computed d2 of a face that
 * lies in no cell of the shells 0 .. r from below and does not ask whether that face is a candidate, so it carries over with
 * "eligible" in front of "face": an unseen eligible face cannot win or tie.  The constant is the same 64 * 2^-23 * m and so is the
 * refusal of a cell below NGP_MESHNORMAL_MIN_CELL_SLACKS * slack(M_grid).
 *
 * THE CAP.  One thing is new with a filter: a query can have no eligible face anywhere, and the first exit then never fires.
 * Under an unbounded max_dist it would walk the whole grid, up to 2^30 cells.  So max_dist must be finite, >= 0 and at most
 * (float)NGP_MESHNORMAL_MAX_SHELLS * cell (NGP_EINVAL otherwise), with oriented == 0 too: the rule is one rule.  A query whose
 * coordinates are no larger in magnitude than M_grid has s_q <= cell / 8, so the second exit ends its walk after shell 9 at the
 * latest (9 cell - cell / 8 > 8 cell): at most 19^3 cells.  A point farther out than M_grid has a larger s_q and may walk on
 * until the third exit; the texels of an atlas, which lie on a mesh within max_dist of the detail mesh, are not such points, and
 * the Python layer (transfer_normals) answers a point beyond (2^14 + 8) cells, up to which the walk still ends after shell 9, as
 * a query that is not valid.  The library itself looks at every finite point it is given, as the rule says.
 */
#ifndef NGP_MESHNORMAL_H
#define NGP_MESHNORMAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef NGP_EINVAL
#define NGP_EINVAL   (-1)  /* bad argument (null pointer, negative size, size or parameter out of range, not finite) */
#endif
#ifndef NGP_ERANGE
#define NGP_ERANGE   (-5)  /* more than INT32_MAX queries, vertices, faces, grid entries or pixels in one call */
#endif

#define NGP_MESHNORMAL_MAX_SHELLS 8          /* max_dist <= 8 * cell */
#define NGP_MESHNORMAL_MAX_AXIS 1024         /* cells per axis of the grid */
#define NGP_MESHNORMAL_MAX_CELLS 1073741824  /* cells of the grid, 2^30 */
#define NGP_MESHNORMAL_SLACK_ULPS 64         /* slack(m) = 64 * 2^-23 * m */
#define NGP_MESHNORMAL_MIN_CELL_SLACKS 8     /* cell >= 8 * slack(M_grid) */
#define NGP_MESHNORMAL_SCAN_BLOCK 2048       /* cells per 8-byte block sum at the head of the grid's workspace */

/* ABI version of this library (1). */
int ngp_meshnormal_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshnormal_build_arch(void);

/* Rules 1 to 4 for n queries against the detail mesh whose grid ngp_meshdist_grid_count / _fill built (same mesh, origin, cell,
 * axes and workspace).  normals_out (n, 3) f32, d2 (n) f32 and face (n) i32 are written for every query; bary (n, 2) f32 or NULL;
 * debug (n, 2) i32 or NULL receives the shells visited and the faces evaluated (rule 2 run) by each query.  entries may be NULL
 * when n_entries == 0.  With n == 0 nothing is launched, but every other argument is still checked.  NGP_EINVAL for a null pointer
 * with a positive size, a negative size, an axis outside [1, 1024], more than 2^30 cells, an origin or cell that is not finite,
 * cell <= 0, a cell below the ratio of THE GRID, a workspace that is too small or not 8-byte aligned, and a max_dist that is not
 * finite, is negative or is above NGP_MESHNORMAL_MAX_SHELLS * cell (THE CAP); NGP_ERANGE for more than INT32_MAX queries,
 * vertices, faces or entries. */
int ngp_meshnormal_transfer(const float* points, const float* query_normals, const uint8_t* valid, int64_t n, const float* vertices,
                            const int32_t* faces, const float* vertex_normals, int64_t n_vertices, int64_t n_faces, const float* origin,
                            float cell, int nx, int ny, int nz, const void* workspace, size_t workspace_bytes, const int32_t* entries,
                            int64_t n_entries, float max_dist, int oriented, float* normals_out, float* d2, int32_t* face, float* bary,
                            int32_t* debug, void* stream);

/* Rule 5 for n_cams frames of H x W pixels: albedo and samples (n_cams, H, W, 3) f32, ids (n_cams, H, W) i32, lights (n_cams, 3)
 * f32 on the DEVICE (unit, pointing towards the light), out (n_cams, H, W, 3) f32 (a buffer of its own).  ambient in [0, 1].
 * n_cams == 0 launches nothing.  NGP_EINVAL for a null pointer with n_cams > 0, a negative n_cams, W or H outside [1, 16384] or an
 * ambient outside [0, 1] (a NaN included); NGP_ERANGE for more than INT32_MAX pixels. */
int ngp_meshnormal_shade(const float* albedo, const float* samples, const int32_t* ids, const float* lights, int64_t n_cams, int H,
                         int W, float ambient, float* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
