/*
 * ngp_meshquadric.h -- C ABI of libngp_meshquadric.so: quadric placement of the vertices of a vertex clustering
 * (Lindstrom's placement for clustering, after Garland and Heckbert's quadric error metric), on gfx950.
 *
 * A library of its own beside libngp_meshsimplify.so (include/ngp_meshsimplify.h), whose vertex_label it consumes, with the
 * conventions of that library and its siblings: raw DEVICE pointers, caller-allocated outputs and workspace, the hipStream_t
 * passed as void*, 0 on success, a positive hipError_t if a launch failed, a negative NGP_E* code for bad arguments.  No entry
 * point allocates or synchronises, and every argument is checked on the host before anything is launched.  This header needs none
 * of the others and may be included before or after them.
 *
 * Mesh: vertices (n_vertices, 3) f32, faces (n_faces, 3) i32.  vertex_label (n_vertices) i32 as ngp_meshsimplify_cluster writes
 * it for the same vertices, origin (3 f32 in DEVICE memory) and cell (a host float, finite and > 0): the smallest vertex index of
 * the vertex's cluster, -1 outside the grid.
 *
 * THE RULE.  f32 operations are IEEE binary32 and f64 operations IEEE binary64, one rounding per operation, no fused
 * multiply-add, division and sqrt correctly rounded.  rint is to nearest even.  (double) of an int64 rounds once, to nearest even.
 *   Q = 1048576 (2^20)     S = 16777216 (2^24)     W_MAX = 16     EPS = 2^-10
 *
 *   The cell c_k, the fraction q_k and OUTSIDE THE GRID of a vertex are those of ngp_meshsimplify.h, recomputed in f32 from
 *   vertices, origin and cell exactly as there.  The coordinates of a cluster are cell units centred on the cell:
 *     y_k = (double)q_k / Q - 0.5                                 (-0.5 <= y_k <= 0.5)
 *
 *   Per cluster, indexed by its label, 14 int64 sums: n, P_0..2, A_00, A_01, A_02, A_11, A_12, A_22, B_0..2, Wsum, in this order.
 *
 *   Member sums.  A vertex v with vertex_label[v] inside [0, n_vertices) that is not outside the grid adds to its label's
 *     n += 1,  P_k += q_k.
 *   Every other vertex adds nothing.
 *
 *   Corner sums.  Every face (i_0, i_1, i_2) contributes once per corner j = 0, 1, 2, with a = i_j, b = i_(j+1 mod 3),
 *   c = i_(j+2 mod 3), to the cluster vertex_label[a].  The corner is SKIPPED when one of the three indices is outside
 *   [0, n_vertices), when vertex_label[a] is outside [0, n_vertices) or when vertex a is outside the grid.  Otherwise, in f64, with
 *   x the f32 vertices converted:
 *     e1 = x_b - x_a,  e2 = x_c - x_a
 *     cr_0 = e1_1 * e2_2 - e1_2 * e2_1,  cr_1 = e1_2 * e2_0 - e1_0 * e2_2,  cr_2 = e1_0 * e2_1 - e1_1 * e2_0
 *     L = sqrt((cr_0 * cr_0 + cr_1 * cr_1) + cr_2 * cr_2)
 *   The corner is SKIPPED unless L is finite and > 0 (repeated indices, zero-area faces, NaN or Inf vertices).  Otherwise
 *     n_k = cr_k / L
 *     w   = min((0.5 * L) / ((double)cell * (double)cell), W_MAX)         the face's area in cells, capped
 *     d   = (n_0 * y_0 + n_1 * y_1) + n_2 * y_2                           y of vertex a: the plane through a is n . y = d
 *   and ten int64 adds to the cluster:
 *     A_ij += (int64) rint(((w * n_i) * n_j) * S)                         for the six i <= j
 *     B_i  += (int64) rint(((w * d) * n_i) * S)
 *     Wsum += (int64) rint(w * S)
 *   Every term is at most 2^28 in magnitude and a cluster has fewer than 3 * 2^31 corners: every sum stays below 2^61.  Reversing a
 *   face's orientation swaps e1 and e2 of each of its corners, which negates cr, n and d exactly and leaves all ten terms as they
 *   are; integer adds commute: the sums depend neither on the orientation of a face nor on the order of the faces.
 *
 *   Placement.  A LEADER is a vertex v with vertex_label[v] == v that is not outside the grid (so n >= 1); c_k is its cell.
 *     m_k = ((double)P_k / (double)n) / Q - 0.5                           the mean, in the cluster's coordinates
 *   If Wsum == 0 the cluster is MEAN_NO_FACES.  Otherwise
 *     r = EPS * (double)Wsum
 *     M_ij = (double)A_ij, plus r on the diagonal;   g_k = (double)B_k + r * m_k
 *   and M y = g is solved by LDL^T without pivoting, in this order:
 *     d0 = M00;  l10 = M01 / d0;  l20 = M02 / d0
 *     d1 = M11 - l10 * M01
 *     t  = M12 - l20 * M01;  l21 = t / d1
 *     d2 = (M22 - l20 * M02) - l21 * t
 *     z0 = g0;  z1 = g1 - l10 * z0;  z2 = (g2 - l20 * z0) - l21 * z1
 *     y2 = z2 / d2;  y1 = z1 / d1 - l21 * y2;  y0 = (z0 / d0 - l10 * y1) - l20 * y2
 *   The cluster is QUADRIC when d0 > 0, d1 > 0, d2 > 0, the three y_k are finite and every |y_k| <= 1 (at most half a cell
 *   beyond the cluster's own cell); its position is
 *     position_k = (float)((double)origin_k + ((double)c_k + (y_k + 0.5)) * (double)cell)
 *   Otherwise it is MEAN_OUTSIDE.  Both MEAN_* states take the expression of ngp_meshsimplify.h,
 *     position_k = (float)((double)origin_k + ((double)c_k + ((double)P_k / (double)n) / Q) * (double)cell)
 *   which is bit for bit the position ngp_meshsimplify_emit gives the cluster.
 *
 *   The term r (I y - m) is the regulariser that stands in place of an SVD with a threshold: M is positive definite with a
 *   condition number of at most about 1 / EPS; on a flat patch the in-plane position is the mean's; perpendicular to a plane of
 *   weight W_i the residual is about EPS * (Wsum / W_i) * |m - plane|.
 *
 * Integer atomic adds only, and one thread per cluster for the placement: every output is bit-identical run to run and for any
 * launch shape.  No kernel reads or writes through an out-of-range index, whatever faces and vertex_label hold.
 */
#ifndef NGP_MESHQUADRIC_H
#define NGP_MESHQUADRIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef NGP_EINVAL
#define NGP_EINVAL   (-1)  /* bad argument (null pointer, negative size, size out of range, workspace too small) */
#endif
#ifndef NGP_ERANGE
#define NGP_ERANGE   (-5)  /* more than INT32_MAX vertices or faces: the indices and counts do not fit int32 */
#endif

#define NGP_MESHQUADRIC_SUMS 14            /* int64 sums per cluster */
#define NGP_MESHQUADRIC_NOT_LEADER    0    /* the values of `state` */
#define NGP_MESHQUADRIC_QUADRIC       1
#define NGP_MESHQUADRIC_MEAN_NO_FACES 2
#define NGP_MESHQUADRIC_MEAN_OUTSIDE  3

/* ABI version of this library (1). */
int ngp_meshquadric_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshquadric_build_arch(void);

/* Device workspace of the three calls below, 256-byte aligned: the 14 int64 sums per vertex (112 B), at least 256 B.  Faces need
 * none.  0 if a size is out of range (negative, or above INT32_MAX). */
size_t ngp_meshquadric_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* Clears the sums, then the member sums and the corner sums of THE RULE into the workspace, indexed by label.  faces may be NULL
 * when n_faces == 0.  With n_vertices == 0 nothing is launched and nothing is written. */
int ngp_meshquadric_accumulate(const float* vertices, const int32_t* faces, const int32_t* vertex_label, int64_t n_vertices,
                               int64_t n_faces, const float* origin, float cell, void* workspace, size_t workspace_bytes, void* stream);

/* After ngp_meshquadric_accumulate with the same n_vertices and workspace: a white-box hook for tests, which compare integers.
 * sums_out (n_vertices, 14) i64: row v holds the sums of THE RULE, in its order, when vertex_label[v] == v, and zeros otherwise.
 * With n_vertices == 0 nothing is launched and nothing is written. */
int ngp_meshquadric_sums(const int32_t* vertex_label, int64_t n_vertices, const void* workspace, size_t workspace_bytes, int64_t* sums_out,
                         void* stream);

/* After ngp_meshquadric_accumulate with the same vertices, vertex_label, n_vertices, origin, cell and workspace: the placement of
 * THE RULE.  positions (n_vertices, 3) f32 is written at leaders only; state (n_vertices) u8 everywhere, one of
 * NGP_MESHQUADRIC_*; totals, DEVICE int64[3], the numbers of clusters that are QUADRIC, MEAN_NO_FACES and MEAN_OUTSIDE.
 * With n_vertices == 0 nothing is launched and nothing is written. */
int ngp_meshquadric_place(const float* vertices, const int32_t* vertex_label, int64_t n_vertices, const float* origin, float cell,
                          const void* workspace, size_t workspace_bytes, float* positions, uint8_t* state, int64_t* totals, void* stream);

#ifdef __cplusplus
}
#endif

#endif
