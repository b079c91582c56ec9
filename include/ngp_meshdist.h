/*
 * ngp_meshdist.h -- C ABI of libngp_meshdist.so: the geometric distance between two indexed triangle meshes on gfx950.  A
 * deterministic area sampler of a mesh's surface, the nearest face of a target mesh for every query point (exactly the brute-force
 * minimum, found through a uniform grid), and the weighted statistics behind Chamfer, Hausdorff and F-score figures.
 *
 * A library of its own beside libngp_hip.so (include/ngp_hip.h), the seven mesh libraries (include/ngp_mesh*.h) and
 * libngp_metrics.so (include/ngp_metrics.h), with their conventions: raw DEVICE pointers, caller-allocated outputs and workspace,
 * the hipStream_t passed as void*, 0 on success, a positive hipError_t if a launch failed, a negative NGP_E* code for bad
 * arguments.  No entry point allocates or synchronises, and every argument is checked on the host before anything is launched.
 * `origin` and `thresholds` are HOST pointers and are read during the call.  This header needs none of the other nine and may be
 * included before or after them.
 *
 * Mesh: vertices (n_vertices, 3) f32, faces (n_faces, 3) i32; vertices may be NULL with n_vertices == 0 and faces with
 * n_faces == 0 (a null pointer with a positive size is NGP_EINVAL).  A face is USABLE when its three indices are inside
 * [0, n_vertices) and its nine coordinates are finite.
 *
 * THE RULE.  Every f32 expression below is IEEE binary32, evaluated in the order written, left to right, each operation rounded
 * on its own (no fused multiply-add); divisions and square roots are correctly rounded.  (float)n of an integer n < 2^24 is
 * exact.  dot(x, y) = (x.x * y.x + x.y * y.y) + x.z * y.z.  x - y, x + y and s * x of vectors act per component.
 *
 * 1. SURFACE SAMPLES.  For a usable face (A, B, C) and spacing > 0:
 *      AB = B - A,  AC = C - A,  BC = C - B
 *      longest = max(max(sqrt(dot(AB, AB)), sqrt(dot(AC, AC))), sqrt(dot(BC, BC)))
 *      c = ceil(longest / spacing);   k = 1 if not (c >= 1),  NGP_MESHDIST_K_MAX if c >= NGP_MESHDIST_K_MAX,  else (int)c
 *    The face is cut into k * k similar sub-triangles and gives k * k samples, one per sub-triangle s in [0, k * k): with
 *    r = isqrt(s) (the row, counted from A), col = s - r * r in [0, 2r], t = col / 2 (integer division), the barycentric integers are
 *      col even (pointing up):    i = 3 (k - r) - 2,  j = 3 (r - t) + 1,  l = 3 t + 1
 *      col odd  (pointing down):  i = 3 (k - r) - 1,  j = 3 (r - t) - 1,  l = 3 t + 2
 *    (i + j + l = 3k; the sub-triangle's centroid), and per component x:
 *      point.x = (((float)i * A.x + (float)j * B.x) + (float)l * C.x) / (float)(3 k)
 *    Its weight is the sub-triangle's area:
 *      n = (AB.y * AC.z - AB.z * AC.y,  AB.z * AC.x - AB.x * AC.z,  AB.x * AC.y - AB.y * AC.x)
 *      weight = (0.5f * sqrt(dot(n, n))) / (float)(k * k)
 *    A face that is not usable gives no samples.  The per-face counts are scanned on the device as integers; the samples are
 *    written in face order and, inside a face, in order of s, each with its face index.  No random numbers.
 *
 * 2. POINT TO TRIANGLE (C. Ericson, Real-Time Collision Detection, 5.1.5).  The closest point q of triangle (a, b, c) to p; the
 *    first case that holds decides:
 *      ab = b - a,  ac = c - a,  ap = p - a,  d1 = dot(ab, ap),  d2 = dot(ac, ap)
 *      vertex a:   d1 <= 0 and d2 <= 0                          q = a
 *      bp = p - b,  d3 = dot(ab, bp),  d4 = dot(ac, bp)
 *      vertex b:   d3 >= 0 and d4 <= d3                         q = b
 *      vc = d1 * d4 - d3 * d2
 *      edge ab:    vc <= 0 and d1 >= 0 and d3 <= 0              v = d1 / (d1 - d3),  q = a + v * ab
 *      cp = p - c,  d5 = dot(ab, cp),  d6 = dot(ac, cp)
 *      vertex c:   d6 >= 0 and d5 <= d6                         q = c
 *      vb = d5 * d2 - d1 * d6
 *      edge ac:    vb <= 0 and d2 >= 0 and d6 <= 0              w = d2 / (d2 - d6),  q = a + w * ac
 *      va = d3 * d6 - d5 * d4
 *      edge bc:    va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0    w = (d4 - d3) / ((d4 - d3) + (d5 - d6)),  q = b + w * (c - b)
 *      interior:   denom = 1 / ((va + vb) + vc),  v = vb * denom,  w = vc * denom,
 *                  v = 0 if not (v >= 0),  v = 1 if v > 1,  w = 0 if not (w >= 0),  w = 1 - v if w > 1 - v,
 *                  q = (a + v * ab) + w * ac
 *    The four clamps of the interior case change nothing in real arithmetic (there 0 < v, 0 < w, v + w < 1); they are what
 *    makes the computed q a point of the triangle whatever rounding did to the signs of va, vb and vc, on which the bound below
 *    rests.  Then
 *      e = p - q,  d2 = (e.x * e.x + e.y * e.y) + e.z * e.z            (the squared distance; not the d2 of the dot products)
 *    A face that is not usable, or whose squared distance is not finite, contributes nothing.
 *
 * 3. THE QUERY.  For a query point p the result is the minimum of the 64-bit key  bits(d2) << 32 | face  over all contributing
 *    faces of the target (d2 >= 0 orders like its bits): the nearest face, and the smaller index where d2 is bit-equal.  The
 *    result is (d2, face) = (+inf, -1), a MISS, if no face contributes or if the minimum d2 > max_dist * max_dist (one f32
 *    product; max_dist may be +inf).  The optional closest point is q of the winning face, recomputed by rule 2, and three NaNs
 *    for a miss.  This is by definition the brute-force minimum over every face: the grid below never changes a bit of it.
 *
 * 4. STATISTICS.  From d2 (n) f32, face (n) i32, weights (n) f32 and T <= 8 thresholds tau, over the elements i with face >= 0,
 *    with w = (double)weights[i], d = sqrt(d2[i]) in f32:
 *      out[0] = sum of w      out[1] = sum of w * (double)d      out[2] = sum of w * (double)d2[i]      out[3] = max of (double)d
 *    over the elements with face < 0 (the misses, left out of the above):  out[4] = sum of w,  out[5] = their number
 *      out[6 + t] = sum of w over the elements with face >= 0 and d2[i] <= tau_t * tau_t (one f32 product), t < T; 0 for t >= T.
 *    Order of the sums: B = min(ceil(n / 256), NGP_MESHDIST_STATS_MAX_BLOCKS) workgroups of 256 threads; thread g of all adds its
 *    elements g, g + 256 B, ... in f64 in that order; the 64 lanes of a wave are added through the shuffle tree
 *    (off = 32, 16, ..., 1: lane l += lane l + off); the four waves of a workgroup in index order; one partial per workgroup; a
 *    second kernel of one wave adds the partials (lane l the partials l, l + 64, ... in index order, then the same tree).  No
 *    float atomics: the same inputs give the same 64 bits.
 *
 * THE GRID (an acceleration; it is not part of the rule).  nx x ny x nz cubic cells of edge `cell`, the first at `origin`; cell
 * (x, y, z) has the index (z * ny + y) * nx + x.  The cell of a coordinate t on an axis with n cells and origin o is
 *      g = floor((t - o) / cell);   0 if not (g >= 0),  n - 1 if g >= n,  else (int)g                    (clamped into the grid)
 * A usable face is entered into every cell of the index box [cell(min - s_f), cell(max + s_f)] per axis, min and max over its
 * three vertices, s_f = slack(max(M_grid, the largest |coordinate| of the face)).  A query visits the Chebyshev shells
 * r = 0, 1, 2, ... of cells around its own (clamped) cell, evaluates rule 2 on every face listed there, and stops after shell r
 * when, with rc = (float)r * cell and s_q = slack(max(M_grid, the largest |coordinate| of p)),
 *      sqrt(best d2) + s_q <= rc,   or   rc - s_q > max_dist,   or   shell r + 1 holds no cell of the grid.
 * A query with a coordinate that is not finite is a miss at once (every d2 is NaN).
 *
 * SLACK.  slack(m) = NGP_MESHDIST_SLACK_ULPS * 2^-23 * m = 2^-17 m, and M_grid = the largest of |origin| and
 * |origin + n * cell| over the three axes.  With u = 2^-24 and M = the largest |coordinate| among p, the face and M_grid:
 *   (a) q.  In the vertex cases q is a vertex.  In the edge cases the inequalities give 0 <= v <= 1 after rounding (d1 >= 0 and
 *       -d3 >= 0 make d1 - d3 >= d1), so q* = a + v * ab (exact, with the computed v) is a point of the edge, and the computed q
 *       differs from it per component by at most 2u |ab| (the difference and the product) + u |q| <= 5 u M.  In the interior case
 *       the clamps give v >= 0, w >= 0, v + w <= 1 + u, so q* = a + v ab + w ac is within u |ac| <= 2 u M of the triangle, and the
 *       computed q differs from q* by at most 2u |ab| + 2u |ac| + u |a + v ab| + u |q| <= 10 u M: 12 u M per component in all,
 *       12 sqrt(3) u M < 21 u M in length.
 *   (b) e = p - q: one rounding of a component of magnitude <= 2M, 2 sqrt(3) u M < 3.5 u M in length.
 *   (c) d2: three products and two sums of non-negative terms, relative error 3u; its square root 1.5u, the rounding of the root
 *       u; |e| <= 2 sqrt(3) M: 2.5 u * 3.47 M < 9 u M.
 *   So sqrt(computed d2) >= dist(p, triangle) - E with E = 33 u M.  (Only this side is needed.  The other side also depends on
 *   the triangle's shape: a case is decided wrongly only when one of va, vb, vc, |value| <= about 20 u L^2 D^2 with L the longest
 *   edge and D the largest |p - vertex|, has the wrong sign, which moves q by at most about 4 * 5 u L^3 D^2 / area^2 along the
 *   triangle and never by more than L.  tests/mesh_distance_reference.py holds the f32 rule to
 *   dist <= computed <= dist + 2E + min(L, 32 u L^3 D^2 / area^2).)
 *   (d) cells.  (t - o) / cell carries two roundings: the coordinate may be taken for one up to delta = 2u |t - o| <= 4 u M
 *       away, so a point lies within delta of its computed cell on every axis where it was not clamped, and a face's index box
 *       covers its padded box moved by at most delta.
 *   (e) a face in no cell of the shells 0 .. r.  Its index box and the cube of radius r around the query's cell are disjoint on
 *       some axis, say i0 >= cx + r + 1 (clamping cannot produce this: an i0 clamped up is 0, a cx clamped down is n - 1).  Then
 *       min - s_f >= o + i0 cell - delta and p <= o + (cx + 1) cell + delta (p clamped up lies lower still), so every point of
 *       the face is at least r cell + s_f - 2 delta from p, and sqrt(its computed d2) >= r cell + s_f - 2 delta - E.
 *   (f) the test sqrt(best d2) + s_q <= rc is made with rc and the sum rounded once each, values <= 4M: rho = 8 u M.
 *   An unseen face cannot win or tie when r cell + s_f - 2 delta - E > r cell - s_q + rho, that is s_f + s_q > 2 delta + E + rho
 *   = (8 + 33 + 8) u M = 49 u M = 24.5 * 2^-23 M.  s_f + s_q >= slack(M) = 64 * 2^-23 M: the multiple is 64, 2.6 times what the
 *   bound asks.  The same margin covers the exit on max_dist (the unseen faces are farther than max_dist + 79 u M, the product
 *   max_dist * max_dist is off by u of itself).  The derivation does not use the size of a cell, but it takes the quotient of (d)
 *   below 2^24 and the padding below a cell: a call with  cell < NGP_MESHDIST_MIN_CELL_SLACKS * slack(M_grid) = 2^-14 M_grid  is
 *   refused (NGP_EINVAL); there the padded boxes would be mostly padding and the exit test would give away more than 1/8 of
 *   every shell.  The bound in (e) holds for points outside the grid too: clamping moves a point towards every cell.
 *   All of this is real arithmetic about f32 values; it assumes no overflow: |coordinate| < 2^60.
 */
#ifndef NGP_MESHDIST_H
#define NGP_MESHDIST_H

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

#define NGP_MESHDIST_K_MAX 64                /* sub-triangles along a face's edge, at most */
#define NGP_MESHDIST_MAX_AXIS 1024           /* cells per axis of the grid */
#define NGP_MESHDIST_MAX_CELLS 1073741824    /* cells of the grid, 2^30 */
#define NGP_MESHDIST_MAX_THRESHOLDS 8
#define NGP_MESHDIST_SLACK_ULPS 64           /* slack(m) = 64 * 2^-23 * m */
#define NGP_MESHDIST_MIN_CELL_SLACKS 8       /* cell >= 8 * slack(M_grid) */
#define NGP_MESHDIST_SCAN_BLOCK 2048         /* elements per workgroup of the integer scans (faces, cells) */
#define NGP_MESHDIST_STATS_MAX_BLOCKS 512    /* workgroups of 256 threads of the statistics */
#define NGP_MESHDIST_STATS_OUTPUTS 14        /* doubles ngp_meshdist_stats writes */

/* ABI version of this library (1). */
int ngp_meshdist_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshdist_build_arch(void);

/* Host only.  *slack = slack(M_grid) and *min_cell = NGP_MESHDIST_MIN_CELL_SLACKS * slack(M_grid) of the grid (SLACK above), both
 * in f32.  NGP_EINVAL for a null pointer, an origin or cell that is not finite, cell <= 0 or an axis outside [1, 1024]. */
int ngp_meshdist_slack(const float* origin, float cell, int nx, int ny, int nz, float* slack, float* min_cell);

/* Bytes of workspace of ngp_meshdist_sample_count / _emit: 4 per face (its count), 8 per face + 8 (its offset) and 8 per block of
 * NGP_MESHDIST_SCAN_BLOCK faces.  0 if n_faces is outside [1, INT32_MAX]. */
size_t ngp_meshdist_sample_workspace_bytes(int64_t n_faces);

/* Sampler pass 1 (rule 1): the per-face counts k * k and their scan.  total: DEVICE int64[1] = the number of samples; the caller
 * reads it once to size the outputs of ngp_meshdist_sample_emit.  workspace: device, 8-byte aligned.  n_faces == 0 launches
 * nothing and writes nothing.  NGP_EINVAL for a null pointer, a negative size, a spacing that is not > 0 and finite, or a
 * workspace that is too small or misaligned; NGP_ERANGE for more than INT32_MAX vertices or faces. */
int ngp_meshdist_sample_count(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float spacing,
                              void* workspace, size_t workspace_bytes, int64_t* total, void* stream);

/* Sampler pass 2 (after ngp_meshdist_sample_count with the same mesh, spacing and workspace): points (n_samples, 3) f32, weights
 * (n_samples) f32 and face_ids (n_samples) i32.  n_samples is the total of pass 1 and the capacity of the outputs: nothing is
 * written past it.  n_samples == 0 launches nothing.  NGP_ERANGE for n_samples above INT32_MAX. */
int ngp_meshdist_sample_emit(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float spacing,
                             void* workspace, size_t workspace_bytes, int64_t n_samples, float* points, float* weights,
                             int32_t* face_ids, void* stream);

/* Bytes of the grid's workspace: 4 per cell (count, then fill cursor), 4 per cell + 4 (the start of every cell's list) and 8 per
 * block of NGP_MESHDIST_SCAN_BLOCK cells.  0 if an axis is outside [1, 1024] or the cells number more than 2^30. */
size_t ngp_meshdist_grid_workspace_bytes(int nx, int ny, int nz);

/* Grid pass 1 (THE GRID): counts the entries of every cell and scans them.  origin: HOST float[3].  total: DEVICE int64[1] = the
 * number of entries; the caller reads it once to size `entries`.  n_faces == 0 is allowed (every list is empty).  NGP_EINVAL for a
 * null pointer, a negative size, an axis outside [1, 1024], more than 2^30 cells, an origin or cell that is not finite, cell <= 0,
 * cell below the ratio of SLACK, or a workspace that is too small or misaligned; NGP_ERANGE for more than INT32_MAX vertices or
 * faces. */
int ngp_meshdist_grid_count(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, const float* origin,
                            float cell, int nx, int ny, int nz, void* workspace, size_t workspace_bytes, int64_t* total, void* stream);

/* Grid pass 2 (after ngp_meshdist_grid_count with the same arguments): entries (n_entries) i32, the face indices of cell c at
 * [start[c], start[c + 1]) in an order that may differ from run to run (a minimum does not depend on it).  n_entries is the total
 * of pass 1.  n_entries == 0 launches nothing.  NGP_ERANGE for n_entries above INT32_MAX. */
int ngp_meshdist_grid_fill(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, const float* origin,
                           float cell, int nx, int ny, int nz, void* workspace, size_t workspace_bytes, int64_t n_entries,
                           int32_t* entries, void* stream);

/* The query (rule 3) for n_points points (n_points, 3) f32 against the mesh whose grid passes 1 and 2 built (same mesh, origin,
 * cell, axes and workspace).  d2 (n_points) f32 and face (n_points) i32 are written for every point; closest (n_points, 3) f32
 * or NULL; debug (n_points, 2) u32 or NULL receives the shells visited and the faces evaluated by each query.  max_dist >= 0,
 * +inf allowed.  entries may be NULL when n_entries == 0.  n_points == 0 launches nothing.  NGP_EINVAL as in grid pass 1, and for a
 * max_dist that is NaN or negative; NGP_ERANGE for more than INT32_MAX points or entries. */
int ngp_meshdist_query(const float* points, int64_t n_points, const float* vertices, const int32_t* faces, int64_t n_vertices,
                       int64_t n_faces, const float* origin, float cell, int nx, int ny, int nz, float max_dist, const void* workspace,
                       size_t workspace_bytes, const int32_t* entries, int64_t n_entries, float* d2, int32_t* face, float* closest,
                       uint32_t* debug, void* stream);

/* Bytes of workspace of ngp_meshdist_stats for n elements: NGP_MESHDIST_STATS_OUTPUTS * 8 per workgroup partial.  0 if n is
 * outside [1, INT32_MAX]. */
size_t ngp_meshdist_stats_workspace_bytes(int64_t n);

/* out: DEVICE double[NGP_MESHDIST_STATS_OUTPUTS] (rule 4).  thresholds: HOST float[n_thresholds], each >= 0 and not NaN, or NULL
 * with n_thresholds == 0.  n >= 1.  NGP_EINVAL for a null pointer, n < 1, n_thresholds outside [0, 8], a bad threshold, or a
 * workspace that is too small or misaligned; NGP_ERANGE for n above INT32_MAX. */
int ngp_meshdist_stats(const float* d2, const int32_t* face, const float* weights, int64_t n, const float* thresholds,
                       int n_thresholds, void* workspace, size_t workspace_bytes, double* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
