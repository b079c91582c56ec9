/*
 * ngp_meshsimplify.h -- C ABI of libngp_meshsimplify.so: simplification of an indexed triangle mesh by vertex clustering on a
 * uniform grid, on gfx950.
 *
 * A library of its own beside libngp_hip.so (include/ngp_hip.h), libngp_mesh.so (include/ngp_mesh.h), libngp_meshfilter.so
 * (include/ngp_meshfilter.h) and libngp_meshcull.so (include/ngp_meshcull.h), with their conventions: raw DEVICE pointers,
 * caller-allocated outputs and workspace, the hipStream_t passed as void*, 0 on success, a positive hipError_t if a launch failed,
 * a negative NGP_E* code for bad arguments.  No entry point allocates or synchronises, and every argument is checked on the host
 * before anything is launched.  This header needs none of the other four and may be included after them.
 *
 * Mesh: vertices (n_vertices, 3) f32, faces (n_faces, 3) i32, optional normals and colors (n_vertices, 3) f32.  The grid: origin,
 * 3 f32 in DEVICE memory (the caller can pass a minimum it computed on the device without reading it back), and cell, the edge of
 * a grid cell, a host float that is finite and > 0.
 *
 * THE RULE.  Q = 1048576 (2^20).  f32 operations are IEEE binary32, one rounding each, no fused multiply-add, the division
 * correctly rounded; f64 operations are IEEE binary64 likewise.  floor() and rint() are the f32 ones, rint to nearest even.
 *
 *   Cell of a vertex x, in f32, per axis k:
 *     t_k = (x_k - origin_k) / cell
 *     c_k = floor(t_k)
 *   The vertex is OUTSIDE THE GRID when some t_k is not finite or some c_k is outside [0, 2^21).  Otherwise
 *     key    = c_0 | c_1 << 21 | c_2 << 42                       (int64)
 *     frac_k = t_k - (float)c_k
 *     q_k    = (int64) rint(frac_k * Q)                           (0 <= q_k <= Q)
 *
 *   Clusters.  All vertices with one key form a cluster, whether or not a face references them.  vertex_label[v] is the SMALLEST
 *   vertex index of v's cluster (the convention of ngp_meshfilter_label), and -1 for a vertex outside the grid.
 *
 *   Cluster attributes.  Exact int64 sums over the n members of the cluster:
 *     P_k = sum q_k
 *     N_k = sum (int64) rint(min(max(normal_k, -1), 1) * Q)       a NaN component contributes 0
 *     C_k = sum (int64) rint(min(max(color_k, 0), 1) * Q)         a NaN component contributes 0
 *   Each is below 2^51 in magnitude (n < 2^31), hence exact as a double.  The outputs, computed in f64 and rounded once to f32:
 *     position_k = (float)((double)origin_k + ((double)c_k + ((double)P_k / (double)n) / Q) * (double)cell)
 *     L          = sqrt(((double)N_0 * (double)N_0 + (double)N_1 * (double)N_1) + (double)N_2 * (double)N_2)
 *     normal_k   = (float)((double)N_k / L),  all three 0 when L == 0
 *     color_k    = (float)(((double)C_k / (double)n) / Q)
 *   The sums are integers because 64-bit integer atomic adds commute and float atomic adds do not: the mean does not depend on
 *   the order in which the members arrive.
 *
 *   Faces.  A face (a, b, c) SURVIVES when its three indices are inside [0, n_vertices), its three labels are >= 0 and its three
 *   labels are pairwise different.  Two surviving faces are DUPLICATES when their label triples are equal as sets (any rotation,
 *   either orientation).  Of a group of duplicates the face with the smallest index is KEPT, as (label_a, label_b, label_c) in its
 *   own order.  A cluster is output when a kept face references it.  Output vertices are in ascending label order; output faces
 *   keep their relative input order and are re-indexed.
 *
 * Keys are claimed by compare-and-swap, the label is an integer minimum, the sums are integer adds, a duplicate group resolves
 * to an integer minimum of face indices and the compaction numbers in index order: every output is bit-identical run to run, for
 * any launch shape and for any capacity of the two hash tables.  No kernel reads or writes through an out-of-range index.
 */
#ifndef NGP_MESHSIMPLIFY_H
#define NGP_MESHSIMPLIFY_H

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

/* ABI version of this library (1). */
int ngp_meshsimplify_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshsimplify_build_arch(void);

/* Device workspace of the three calls below, 256-byte aligned.  With T(n) = the power of two >= 2 n (at least 64, at most 2^31):
 * per vertex the cluster table (12 B x T(n_vertices) / n_vertices: 24 to 48), ten int64 sums (80), the clusters' f32 attributes
 * (36) and the compaction's 5; per face its label triple (12) and the duplicate table (4 B x T(n_faces) / n_faces: 8 to 16); 12 B
 * per block of 2048 vertices and per block of 2048 faces.  The part ngp_meshsimplify_cluster uses does not depend on n_faces:
 * ngp_meshsimplify_workspace_bytes(n_vertices, 0) is enough for that call alone.
 * 0 if a size is out of range (negative, or above INT32_MAX). */
size_t ngp_meshsimplify_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* vertex_label (n_vertices) i32 of THE RULE; the clusters' member counts and integer sums stay in the workspace, indexed by
 * label.  normals and colors may be NULL: their sums are then 0.  origin: DEVICE pointer to 3 f32.  cell: finite and > 0.
 * With n_vertices == 0 nothing is launched and nothing is written. */
int ngp_meshsimplify_cluster(const float* vertices, const float* normals, const float* colors, int64_t n_vertices, const float* origin,
                             float cell, void* workspace, size_t workspace_bytes, int32_t* vertex_label, void* stream);

/* After ngp_meshsimplify_cluster with the same n_vertices and workspace.  Writes every face's label triple, (-1, -1, -1) for one
 * that does not survive; finds the duplicates and keeps the smallest index of each group; marks the clusters the kept faces
 * reference; counts both per block and scans the block counts on the device.  A label outside [-1, n_vertices) is taken as -1.
 * totals: DEVICE int64[3] = {output vertices, output faces, clusters}; the caller reads it once to size the outputs of
 * ngp_meshsimplify_emit.  With n_vertices == 0 nothing is launched and nothing is written. */
int ngp_meshsimplify_count(const int32_t* faces, const int32_t* vertex_label, int64_t n_vertices, int64_t n_faces, void* workspace,
                           size_t workspace_bytes, int64_t* totals, void* stream);

/* After ngp_meshsimplify_count with the same sizes and workspace; vertices, origin and cell are those ngp_meshsimplify_cluster had.
 * The attributes of the output clusters (THE RULE) into vertices_out / normals_out / colors_out (out_vertices, 3) f32 and the kept
 * faces, re-indexed, into faces_out (out_faces, 3) i32.  normals_out / colors_out are NULL when ngp_meshsimplify_cluster had no
 * normals / colors.  out_vertices / out_faces are the totals of ngp_meshsimplify_count and the capacity of the outputs: nothing is
 * written past them. */
int ngp_meshsimplify_emit(const float* vertices, int64_t n_vertices, int64_t n_faces, const float* origin, float cell, void* workspace,
                          size_t workspace_bytes, int64_t out_vertices, int64_t out_faces, float* vertices_out, float* normals_out,
                          float* colors_out, int32_t* faces_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
