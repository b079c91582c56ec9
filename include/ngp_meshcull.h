/*
 * ngp_meshcull.h -- C ABI of libngp_meshcull.so: a depth-buffer visibility test of an indexed triangle mesh against a set of
 * pinhole cameras, and the sub-mesh of the faces that some camera sees, on gfx950.
 *
 * A library of its own beside libngp_hip.so (include/ngp_hip.h), libngp_mesh.so (include/ngp_mesh.h) and libngp_meshfilter.so
 * (include/ngp_meshfilter.h), with their conventions: raw DEVICE pointers, caller-allocated outputs and workspace, the hipStream_t
 * passed as void*, 0 on success, a positive hipError_t if a launch failed, a negative NGP_E* code for bad arguments.  No entry
 * point allocates or synchronises, and every argument is checked on the host before anything is launched.  This header needs none
 * of the other three and may be included after them.
 *
 * Mesh: vertices (n_vertices, 3) f32 in world coordinates, faces (n_faces, 3) i32.  Cameras: poses (n_cams, 3, 4) f32 row-major
 * camera-to-world [R | t], K (3, 3) f32 row-major, images of W x H pixels: the conventions of ngp_mark_invisible_cells.
 *
 * THE RULE.  Every expression below is IEEE binary32, evaluated in the order written, left to right, each operation rounded on
 * its own (no fused multiply-add), divisions correctly rounded; floor() is the f32 floor.
 *
 *   Camera c, with R = poses[c][:, 0:3] and t = poses[c][:, 3]:
 *     m[r][k] = R[k][r]                                         (row r of R^T)
 *     s[r]    = -(m[r][0] * t[0] + m[r][1] * t[1] + m[r][2] * t[2])
 *   A vertex x = (x0, x1, x2):
 *     p[r] = m[r][0] * x0 + m[r][1] * x1 + m[r][2] * x2 + s[r]
 *     ud = K[0][0] * p[0] + K[0][1] * p[1] + K[0][2] * p[2],  vd and d likewise from rows 1 and 2 of K
 *     u = ud / d,  v = vd / d,  q = 1 / d
 *
 *   Raster.  A face (a, b, c) contributes to camera c only when its three indices are inside [0, n_vertices) and its three
 *   vertices have d >= near.  There is no clipping: a face that crosses the near plane occludes nothing, which can only keep too
 *   much.  With the screen points A = (u_a, v_a), B, C and
 *     E_ab(P) = (B.x - A.x) * (P.y - A.y) - (B.y - A.y) * (P.x - A.x)
 *     E_bc(P) = (C.x - B.x) * (P.y - B.y) - (C.y - B.y) * (P.x - B.x)
 *     E_ca(P) = (A.x - C.x) * (P.y - C.y) - (A.y - C.y) * (P.x - C.x)
 *     area    = E_ab(C)
 *   a face with area == 0 or a non-finite area is skipped.  The pixels visited are
 *     i in [max(0, floor(min(u_a, u_b, u_c))), min(W - 1, floor(max(u_a, u_b, u_c)))],  j likewise from v and H,
 *   with the centre P = (i + 0.5, j + 0.5).  With w_a = E_bc(P), w_b = E_ca(P), w_c = E_ab(P) the pixel is covered when all three
 *   are >= 0 (area > 0) or all three are <= 0 (area < 0): every edge is inclusive and either winding is accepted.  Its depth is
 *     z = area / (w_a * q_a + w_b * q_b + w_c * q_c)
 *   and a z that is not finite or not > 0 is dropped.  zbuf[c][j][i] is the MINIMUM z over all faces, formed by a 32-bit unsigned
 *   atomic minimum on the float's bits (z > 0 orders like its bits) from a buffer cleared to the bits of +inf (0x7F800000).
 *
 *   Vertex test.  A vertex HAS A VIEW in camera c when
 *     d >= near  and  0 <= u < W  and  0 <= v < H  and  d <= zbuf[c][floor(v)][floor(u)] + bias.
 *   bias is an absolute distance in world units.  A pixel no face covered holds +inf and passes.
 *
 *   Selection.  vertex_views[x] is the number of cameras in which vertex x has a view.  A face is kept when its indices are in
 *   range and vertex_views >= min_views for at least one of its vertices; a vertex is kept when a kept face references it (its
 *   own test may have failed).  The kept vertices and faces stay in the input's relative order, the faces re-indexed.
 *
 * A minimum does not depend on the order of the writes, vertex_views is a plain per-vertex sum made by the one thread that owns
 * the vertex (no atomic), and the compaction numbers in index order: every output is bit-identical run to run, for any launch
 * shape and for any split of the cameras into chunks.
 */
#ifndef NGP_MESHCULL_H
#define NGP_MESHCULL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef NGP_EINVAL
#define NGP_EINVAL   (-1)  /* bad argument (null pointer, negative size, size out of range, workspace too small) */
#endif
#ifndef NGP_ERANGE
#define NGP_ERANGE   (-5)  /* more than INT32_MAX vertices, faces or cameras: the indices and counts do not fit int32 */
#endif

/* ABI version of this library (1). */
int ngp_meshcull_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshcull_build_arch(void);

/* Bytes of n_cams depth buffers of W x H pixels: 4 * W * H * n_cams.  0 if W or H is outside [1, 16384] or n_cams outside
 * [1, INT32_MAX].  ngp_meshcull_views accepts any workspace that holds at least one camera. */
size_t ngp_meshcull_zbuffer_bytes(int W, int H, int64_t n_cams);

/* Device workspace ngp_meshcull_count / ngp_meshcull_emit need: 5 bytes per vertex (a referenced-by-a-kept-face byte and the int32
 * new index) plus 12 bytes per block of 2048 vertices and per block of 2048 faces (an int32 count and an int64 offset).
 * 0 if a size is out of range (negative, or above INT32_MAX). */
size_t ngp_meshcull_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* vertex_views (n_vertices) i32 = the number of cameras in which each vertex has a view (THE RULE above).  zbuffer is a device
 * workspace of zbuffer_bytes bytes, 4-byte aligned, with room for at least one camera (4 * W * H bytes).  The cameras are processed
 * in chunks of as many as fit: per chunk the buffer is cleared, the faces are rasterised into it and the vertices are tested
 * against it, vertex_views accumulating across the chunks.  near_distance is the rule's `near`.  After a call whose cameras fit
 * one chunk the workspace holds zbuf[c][j][i] as (n_cams, H, W) u32 depth bits.  W and H run from 1 to 16384, n_cams >= 1.
 * With n_vertices == 0 nothing is launched and nothing is written. */
int ngp_meshcull_views(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, const float* K, const float* poses,
                       int64_t n_cams, int W, int H, float near_distance, float bias, void* zbuffer, size_t zbuffer_bytes, int32_t* vertex_views,
                       void* stream);

/* Compaction pass 1.  Marks the kept faces (Selection above, with vertex_views as ngp_meshcull_views wrote it) and the vertices
 * they reference, counts both per block and scans the block counts on the device.  totals: DEVICE int64[2] = {kept vertices, kept
 * faces}; the caller reads it once to size the outputs of ngp_meshcull_emit.
 * With n_vertices == 0 and n_faces == 0 nothing is launched and nothing is written. */
int ngp_meshcull_count(const int32_t* faces, const int32_t* vertex_views, int32_t min_views, int64_t n_vertices, int64_t n_faces,
                       void* workspace, size_t workspace_bytes, int64_t* totals, void* stream);

/* Compaction pass 2 (after ngp_meshcull_count with the same mesh, vertex_views, min_views and workspace): the kept vertices and
 * faces in the input's relative order, the faces re-indexed.  vertices / normals / colors are (n_vertices, 3) f32, copied bit for
 * bit into vertices_out / normals_out / colors_out (out_vertices, 3); normals and colors may be NULL, together with their outputs.
 * faces_out is (out_faces, 3) i32.  out_vertices / out_faces are the totals of ngp_meshcull_count and the capacity of the outputs:
 * nothing is written past them. */
int ngp_meshcull_emit(const int32_t* faces, const int32_t* vertex_views, int32_t min_views, const float* vertices, const float* normals,
                      const float* colors, int64_t n_vertices, int64_t n_faces, void* workspace, size_t workspace_bytes,
                      int64_t out_vertices, int64_t out_faces, float* vertices_out, float* normals_out, float* colors_out,
                      int32_t* faces_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
