/*
 * ngp_meshsmooth.h -- C ABI of libngp_meshsmooth.so: Taubin's lambda|mu smoothing of an indexed triangle mesh on an integer grid,
 * and geometric vertex normals, on gfx950.
 *
 * A library of its own beside libngp_hip.so (include/ngp_hip.h), libngp_mesh.so (include/ngp_mesh.h), libngp_meshfilter.so
 * (include/ngp_meshfilter.h), libngp_meshcull.so (include/ngp_meshcull.h), libngp_meshsimplify.so (include/ngp_meshsimplify.h)
 * and libngp_meshtsdf.so (include/ngp_meshtsdf.h), with their conventions: raw DEVICE pointers, caller-allocated outputs and
 * workspace, the hipStream_t passed as void*, 0 on success, a positive hipError_t if a launch failed, a negative NGP_E* code for
 * bad arguments.  No entry point allocates or synchronises, and every argument is checked on the host before anything is
 * launched.  This header needs none of the other six and may be included before or after them.
 *
 * Mesh: vertices (n_vertices, 3) f32, faces (n_faces, 3) i32.  The grid: origin, 3 f32 in DEVICE memory (the caller can pass a
 * minimum it computed on the device without reading it back), and cell, a host float that is finite and > 0.
 *
 * THE RULE.  Q = 65536, QMAX = 2^30.  f32 and f64 operations are IEEE, one rounding each, no fused multiply-add, the divisions
 * correctly rounded; rint rounds to nearest even; int64 -> f64 conversion rounds to nearest even.
 *
 *   Grid state.  Per vertex x and axis k, in f32:
 *     t_k = (x_k - origin_k) / cell
 *     r_k = rint(t_k * Q)
 *   The vertex is INSIDE when every t_k is finite and every |r_k| <= QMAX; its state is then q_k = (int64) r_k, which fits int32.
 *   An outside vertex has no state and takes no part in smoothing.  With cell = the lattice spacing the quantum is spacing / 65536.
 *
 *   Edges.  A face is VALID when its three indices are inside [0, n_vertices) and pairwise different.  Each valid face has three
 *   sides; a side whose two ends are both inside is one OCCURRENCE of the unordered edge {a, b}, wherever the third corner is.  The
 *   edges are the distinct pairs that occur at least once.  N(v) is the set of the other ends of v's edges, degree[v] = |N(v)|
 *   (0 for an outside vertex).  A BOUNDARY edge occurs exactly once; a BOUNDARY vertex is an end of one.  A vertex is FREE when it is
 *   inside, has degree > 0 and is not a boundary vertex while pin_boundary is set.
 *     flags[v] = 1 (inside) | 2 (boundary) | 4 (free)
 *
 *   A pass with factor f (f64, converted from the f32 argument).  For every free vertex v and axis k, from the states of BEFORE
 *   the pass:
 *     D_k  = sum over u in N(v) of q_k[u]  -  degree[v] * q_k[v]                     exact in int64, |D_k| < 2^62
 *     q'_k = min(max(q_k + (int64) rint(f * ((double)D_k / (double)degree[v])), -QMAX), QMAX)
 *   The states of vertices that are not free do not change; their neighbours still read them.
 *
 *   Taubin.  `pairs` times: a pass with lambda, then a pass with mu.
 *
 *   Output.  For a free vertex x'_k = (float)((double)origin_k + ((double)q_k / Q) * (double)cell); for every other vertex the
 *   input words, bit for bit.  Faces are not touched.
 *
 *   Geometric normals, independent of the grid.  For every face whose indices are inside [0, n_vertices), its corners a, b, c
 *   taken as f64:
 *     e1 = b - a, e2 = c - a
 *     c  = (e1_y * e2_z - e1_z * e2_y,  e1_z * e2_x - e1_x * e2_z,  e1_x * e2_y - e1_y * e2_x)
 *     L  = sqrt((c_0 * c_0 + c_1 * c_1) + c_2 * c_2)
 *   If L > 0 and every c_k / L is finite the face adds (int64) rint((c_k / L) * 2^20) to each of its three corners, otherwise
 *   nothing.  The normal of a vertex is its int64 sum N (below 2^51 in magnitude), normalised in f64 as include/ngp_meshsimplify.h
 *   normalises its N:
 *     L        = sqrt(((double)N_0 * (double)N_0 + (double)N_1 * (double)N_1) + (double)N_2 * (double)N_2)
 *     normal_k = (float)((double)N_k / L),  all three 0 when L == 0
 *   Counter-clockwise faces seen from outside give outward normals.
 *
 * Edge keys are claimed by compare-and-swap, occurrences, degrees and the normals' sums are integer adds, the order inside a
 * neighbour list is arbitrary and only ever feeds an integer sum, every other value is a single expression: all outputs are
 * bit-identical run to run, for any launch shape, any capacity of the edge table and any order of the faces within the same set
 * of faces.  The passes are gathers without atomics.  No kernel reads or writes through an out-of-range index.
 */
#ifndef NGP_MESHSMOOTH_H
#define NGP_MESHSMOOTH_H

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
int ngp_meshsmooth_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshsmooth_build_arch(void);

/* Device workspace of the three calls below, 256-byte aligned.  With T = the power of two >= 6 n_faces (at least 64): per vertex
 * two ping-pong states of 16 B (32), the int64 row offset of the neighbour lists (8), the degree that becomes the fill cursor (4),
 * a copy of the flags (1) and the normals' three int64 sums (24): 69 B; per face the edge table (12 B x T / n_faces: 72 to 144) and
 * the 6 neighbour entries of its three sides (24); 16 B per block of 2048 vertices.  The bounds need no host read: a mesh has at
 * most 3 n_faces edges and 6 n_faces neighbour entries.
 * 0 if a size is out of range (negative, or above INT32_MAX). */
size_t ngp_meshsmooth_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* The edges, the degrees, the flags and the neighbour lists of THE RULE; the lists stay in the workspace.  degree (n_vertices)
 * i32, flags (n_vertices) u8, totals: DEVICE int64[4] = {edges, boundary edges, free vertices, boundary vertices}.  origin:
 * DEVICE pointer to 3 f32.  cell: finite and > 0.  pin_boundary: 0 or not 0.  faces may be NULL when n_faces == 0.
 * With n_vertices == 0 nothing is launched and nothing is written. */
int ngp_meshsmooth_topology(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, const float* origin,
                            float cell, int pin_boundary, void* workspace, size_t workspace_bytes, int32_t* degree, uint8_t* flags,
                            int64_t* totals, void* stream);

/* After ngp_meshsmooth_topology with the same vertices, sizes, grid and workspace.  `pairs` (>= 1) times a pass with lambda and a
 * pass with mu (each finite, magnitude <= 1), one launch per pass, then the output of THE RULE into vertices_out (n_vertices, 3)
 * f32, which must not overlap vertices.  May be called again: it starts from `vertices` every time.
 * With n_vertices == 0 nothing is launched and nothing is written. */
int ngp_meshsmooth_taubin(const float* vertices, int64_t n_vertices, int64_t n_faces, const float* origin, float cell, int pairs,
                          float lambda, float mu, void* workspace, size_t workspace_bytes, float* vertices_out, void* stream);

/* The geometric normals of THE RULE into normals_out (n_vertices, 3) f32.  Independent of the other two calls; it uses a part of
 * the workspace they leave alone.  faces may be NULL when n_faces == 0 (every normal is then 0).
 * With n_vertices == 0 nothing is launched and nothing is written. */
int ngp_meshsmooth_normals(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, void* workspace,
                           size_t workspace_bytes, float* normals_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
