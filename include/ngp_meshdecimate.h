/*
 * ngp_meshdecimate.h -- C ABI of libngp_meshdecimate.so: decimation of a triangle mesh to a face budget or an error bound by
 * rounds of independent half-edge collapses under a plane-distance (quadric) cost, memoryless after Lindstrom and Turk, on gfx950.
 *
 * A library of its own beside its siblings, with their conventions: raw DEVICE pointers, caller-allocated outputs and workspace,
 * the hipStream_t passed as void*, 0 on success, a positive hipError_t if a launch failed, a negative NGP_E* code for bad
 * arguments.  No entry point allocates or synchronises, and every argument is checked on the host before anything is launched.
 * This header needs none of the others and may be included before or after them.
 *
 * Mesh: vertices (n_vertices, 3) f32, faces (n_faces, 3) i32, optional normals and colours (n_vertices, 3) f32.  At most
 * INT32_MAX vertices and INT32_MAX / 3 faces: a corner's number, 3 * face + corner, fits int32.
 *
 * The caller drives the rounds, because each needs one host read:
 *     begin;  repeat { round;  read totals;  stop or apply }  count;  read totals;  emit
 *
 * THE RULE.  f64 operations are IEEE binary64, one rounding per operation, no fused multiply-add, division and sqrt correctly
 * rounded; x_i is the f32 position of vertex i converted to f64.  rint is to nearest even.  (a, b, ...) < (a', b', ...) is the
 * lexicographic order.
 *   MAX_DEGREE = 64     S = 1048576 (2^20)     CAP = 1125899906842624 (2^50)     NONE = 2^64 - 1
 *   KC = S / ((cell * cell) * cell),  KL = S / (cell * cell),  E2 = max_error * max_error        with cell, max_error as f64
 *
 *   Current faces.  begin copies the faces; a face with an index outside [0, n_vertices) or with two equal indices is DEAD from
 *   the start.  Every later step sees only the faces that are not dead; they keep their place and their orientation.
 *
 *   A round is a function of the set of current faces and of the vertices alone.  For a vertex u, its CORNERS are the current
 *   faces that hold u, each written (u, a, b) in the face's cyclic order: a is the next corner, b the previous one.
 *
 *   REMOVABLE.  u is removable when all of these hold:
 *     3 <= the number d of its corners <= MAX_DEGREE;
 *     the three coordinates of u and of every a are finite;
 *     every a occurs in exactly one corner as a, every b in exactly one corner as b, and every b occurs as the a of a corner: the
 *       successor of a corner is the corner whose a is its b;
 *     following successors from any corner returns to it after exactly d steps, not sooner (one closed, oriented fan).
 *   Boundary, non-manifold and bow-tie vertices fail this test, and so does a vertex of a face stored twice.  N(u) is the set of
 *   the a of u's corners.  For any vertex v, N(v) is the set of vertices other than v in the current faces that hold v.
 *
 *   VALID.  For removable u and v in N(u), with dv = x_v - x_u, every corner (u, a, b) with a != v and b != v has
 *     e1 = x_a - x_u,  e2 = x_b - x_u,  f1 = x_a - x_v,  f2 = x_b - x_v
 *     c_0 = e1_1 * e2_2 - e1_2 * e2_1,  c_1 = e1_2 * e2_0 - e1_0 * e2_2,  c_2 = e1_0 * e2_1 - e1_1 * e2_0        (c' from f1, f2 alike)
 *     LL = (c_0 * c_0 + c_1 * c_1) + c_2 * c_2,   L = sqrt(LL)
 *     dot = (c_0 * c'_0 + c_1 * c'_1) + c_2 * c'_2
 *     g = (c_0 * dv_0 + c_1 * dv_1) + c_2 * dv_2
 *   The collapse u -> v is valid when
 *     exactly 2 members w of N(u) other than v lie in N(v)                      (the link condition);
 *     for every such corner dot > 0                                             (the face neither flips nor degenerates);
 *     for every such corner no current face holds the three vertices v, a, b    (the tetrahedron case);
 *     for every such corner, when max_error >= 0,  g * g <= E2 * LL             (v within max_error of the face's plane).
 *   All operands are finite, so no comparison sees a NaN; max_error < 0 switches the last test off.
 *
 *   COST.  cost(u -> v) = the sum over the same corners of (int64) rint(min(((g * g) / L) * KC, CAP)): 2 * area * distance^2 in
 *   units of cell^3 / S.  At most 64 terms of at most 2^50: the sum stays below 2^56, and integer adds commute.
 *     len(u -> v) = (int64) rint(min(((dv_0 * dv_0 + dv_1 * dv_1) + dv_2 * dv_2) * KL, CAP))
 *   The TARGET of u is the valid v with the smallest (cost, len, v).  A removable u with a target is a CANDIDATE.
 *
 *   KEY, narrowed to 64 bits.  code(0) = 0; for c > 0 with highest set bit e (c >> e == 1) and m = c >> (e - 23) if e >= 23,
 *   c << (23 - e) otherwise:  code(c) = ((e + 1) << 23) | (m & 0x7FFFFF): the cost to 24 significant bits, truncated, monotone.
 *     mix(u):  x = (uint32) u * 0x9E3779B1;  x ^= x >> 15;  x *= 0x85EBCA77;  x ^= x >> 13          (uint32 arithmetic, a bijection)
 *     key(u) = ((uint64) code(cost) << 32) | mix(u)
 *   mix is a bijection, so the keys of two vertices differ, the index itself is not needed, and key < NONE.  The edge length
 *   decides between targets only.
 *
 *   WINNERS.  Every vertex has a claim word, NONE at the start of the round.  Every candidate u takes the minimum of its key into
 *   the words of u and of every member of N(u).  u WINS when all of those words hold its key.  Two winners have disjoint closed
 *   one-rings, so no face holds two winners and no winner is another's neighbour; the smallest key of the round always wins.
 *   totals of a round: the number of candidates, the number of winners, the number of current faces.
 *
 *   APPLY.  Of the n_winners winners the n_keep with the smallest keys are APPLIED (all when n_keep == n_winners).  Every index u
 *   of a current face that is an applied winner becomes target(u); a face with two equal indices after that is dead.  Each applied
 *   winner kills exactly the two faces that hold u and its target.  No vertex moves.
 *
 *   The caller's loop, with F the current faces (totals[2]; afterwards F - 2 * applied): stop when target_faces is set and
 *   F <= target_faces, or when the round has no candidate; otherwise apply min(winners, ceil((F - target_faces) / 2)), or all
 *   winners without target_faces.
 *
 *   OUTPUT.  count / emit: the current faces in their order, the vertices they reference in their order, re-indexed; positions,
 *   normals and colours are copied bit for bit.
 *
 * Integer atomics only (add, min), and every float expression is evaluated by one lane in the order above: every output is
 * bit-identical run to run and for any launch shape or face order.  No kernel reads or writes through an out-of-range index,
 * whatever faces holds.
 */
#ifndef NGP_MESHDECIMATE_H
#define NGP_MESHDECIMATE_H

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

#define NGP_MESHDECIMATE_MAX_DEGREE 64     /* a vertex with more corners is never removed */
#define NGP_MESHDECIMATE_MAX_FACES  715827882      /* INT32_MAX / 3; more faces give NGP_ERANGE */

/* ABI version of this library (1). */
int ngp_meshdecimate_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshdecimate_build_arch(void);

/* Device workspace of the calls below, 256-byte aligned: 45 B per vertex and 24 B per face plus block tables, at least 256 B.
 * 0 if a size is out of range (negative, n_vertices above INT32_MAX, n_faces above NGP_MESHDECIMATE_MAX_FACES). */
size_t ngp_meshdecimate_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* Copies the faces into the workspace as the current faces of THE RULE.  With n_faces == 0 nothing is launched. */
int ngp_meshdecimate_begin(const int32_t* faces, int64_t n_vertices, int64_t n_faces, void* workspace, size_t workspace_bytes, void* stream);

/* One round of THE RULE up to WINNERS on the current faces.  cell: finite and > 0.  max_error: finite; negative for no bound.
 * totals, DEVICE int64[3]: candidates, winners, current faces.  With n_vertices == 0 or n_faces == 0 the totals are cleared and
 * nothing else happens. */
int ngp_meshdecimate_round(const float* vertices, int64_t n_vertices, int64_t n_faces, float cell, float max_error, void* workspace,
                           size_t workspace_bytes, int64_t* totals, void* stream);

/* APPLY of THE RULE after ngp_meshdecimate_round with the same sizes and workspace: n_winners as that round reported them,
 * 0 <= n_keep <= n_winners <= n_vertices.  With n_keep == 0 nothing is launched. */
int ngp_meshdecimate_apply(int64_t n_vertices, int64_t n_faces, int64_t n_winners, int64_t n_keep, void* workspace, size_t workspace_bytes,
                           void* stream);

/* The sizes of OUTPUT: totals, DEVICE int64[2] = {vertices, faces}. */
int ngp_meshdecimate_count(int64_t n_vertices, int64_t n_faces, void* workspace, size_t workspace_bytes, int64_t* totals, void* stream);

/* After ngp_meshdecimate_count with the same sizes and workspace, n_out_vertices and n_out_faces being its totals: writes OUTPUT.
 * normals / colors and their outputs may be NULL (both of a pair or neither). */
int ngp_meshdecimate_emit(const float* vertices, const float* normals, const float* colors, int64_t n_vertices, int64_t n_faces,
                          void* workspace, size_t workspace_bytes, int64_t n_out_vertices, int64_t n_out_faces, float* vertices_out,
                          float* normals_out, float* colors_out, int32_t* faces_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
