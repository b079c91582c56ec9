/*
 * ngp_meshchart.h -- C ABI of libngp_meshchart.so: a texture atlas made of charts (connected groups of faces that project onto
 * one coordinate plane without overlap), with the owner of every texel, a padded border round every chart, the world point and
 * viewing direction of every texel, one UV per vertex and chart, and a renderer of the mesh textured that way, on gfx950.
 *
 * A library of its own beside the others, with their conventions: raw DEVICE pointers, caller-allocated outputs and workspace,
 * the hipStream_t passed as void*, 0 on success, a positive hipError_t if a launch failed, a negative NGP_E* code for bad
 * arguments.  No entry point allocates or synchronises, and every argument is checked on the host before anything is launched.
 * This header needs none of the others and may be included before or after them.  It lies beside the library's sources, not
 * under include/.  No other library is changed or needed.
 *
 * Mesh: vertices (n_vertices, 3) f32 in world coordinates, faces (n_faces, 3) i32, normals (n_vertices, 3) f32.  Cameras: poses
 * (n_cams, 3, 4) f32 row-major camera-to-world [R | t], K (3, 3) f32 row-major, images of W x H pixels: the conventions of
 * include/ngp_meshcull.h.  box: six HOST floats lo0 lo1 lo2 hi0 hi1 hi2, finite, lo <= hi.  background: three HOST floats.
 *
 * THE RULE.  Every decision is taken in integers.  f32 operations are IEEE binary32, one rounding each, in the order written, no
 * fused multiply-add; f64 likewise; divisions and square roots are correctly rounded.  >> on a negative integer is the
 * arithmetic shift (floor).
 *
 *   Snap.  texel_size = s (f32, finite, > 0: world units per texel), c = (float)(16.0 / (double)s).  A face with an index outside
 *   [0, n_vertices) has class 6; nothing is read through such an index.  Otherwise, per corner and axis, t = v_k * c (f32); if
 *   a t is not finite or |t| >= 2^22 the face has class 6; otherwise X_k = (int32)rint(t), halves to even: the coordinate in
 *   sixteenths of a texel.
 *
 *   Class.  n = (B - A) x (C - A) in int64 (exact).  k is the axis of the largest |n_k|, the smallest k on a tie.  n_k == 0 gives
 *   class 6 (no chart); otherwise the class is 2 k + (n_k < 0).  The chart plane of a class has the axes (u, v) = ((k + 1) % 3,
 *   (k + 2) % 3), swapped when n_k < 0, and a corner's plane coordinates are (X_u, X_v): every classified face has the strictly
 *   positive area |n_k| = (B_u - A_u)(C_v - A_v) - (B_v - A_v)(C_u - A_u) there.
 *
 *   Vertex table.  vf_offsets (n_vertices + 1) i64 and vf_faces (3 n_faces) i32: the faces with all indices in range, listed
 *   once per corner under that corner's vertex; vf_offsets[n_vertices] entries in all.  The order inside a vertex's list is not
 *   defined and nothing depends on it.
 *
 *   Charts of a stage.  Among the ACTIVE faces (active[f] != 0 and class < 6), two faces are chart-adjacent when they have the
 *   same class and two vertex indices in common; more than two faces on an edge are adjacent pairwise.  A chart is a connected
 *   component; its label is its smallest face index; with unite == 0 every active face is a chart of its own.  The charts of the
 *   stage are numbered chart_base, chart_base + 1, ... by ascending label.  face_label[f] and face_chart[f] are written for the
 *   active faces; face_label is -1 and face_chart is left alone for every other face.
 *
 *   Bounds of a chart: the minimum and the maximum of X_u and of X_v over the corners of its faces, (umin, vmin, umax, vmax).
 *   Rectangle (by the caller, on the host): o = min >> 4 per axis, w = (umax >> 4) - o_u + 1, h likewise, the rectangle is
 *   (w + 2 pad) x (h + 2 pad) texels with 0 <= pad <= 8, and chart_rects (n_charts, 6) i32 holds rx, ry (the rectangle's origin
 *   from the packing), w + 2 pad, h + 2 pad, o_u, o_v.  A corner's atlas coordinate in sixteenths is
 *     x = 16 (rx + pad - o_u) + X_u,   y = 16 (ry + pad - o_v) + X_v
 *   an integer translation.  Texel (i, j) has its centre at (16 i + 8, 16 j + 8); the atlas is row-major, row 0 on top.
 *
 *   Packing, a function of the n rectangles' sizes alone, on the host.  Order (sorted != 0): height descending, then width
 *   descending, then index ascending; (sorted == 0): index ascending.  Shelves: x = 0, y = y0, shelf = 0; for each rectangle in
 *   order: if x + w > W then y += shelf, x = 0, shelf = 0; its origin is (x, y); x += w; shelf = max(shelf, h).  H(W) = y + shelf.
 *   With width_in == 0: W0 = max(widest rectangle, ceil(sqrt(sum of w h))), and while H(W) > W, W += max(1, W >> 4).  With
 *   width_in > 0, W = width_in (a later stage continues below the atlas at the same W, from y0 = the height so far).  W > 16384
 *   or H(W) > 16384 returns NGP_ERANGE.
 *
 *   Ownership.  A face covers the texel centre P when all three edge functions, over the edges p -> q = a -> b, b -> c, c -> a of
 *   its atlas coordinates,
 *     E = dx (P_y - p_y) - dy (P_x - p_x),   dx = q_x - p_x,  dy = q_y - p_y      (int64)
 *   are positive, where E == 0 counts as positive only when dy > 0, or dy == 0 and dx < 0.  The owner of a texel is the smallest
 *   face index among the faces of the stage's charts [chart_lo, chart_hi) that cover it: an unsigned atomic minimum on a map
 *   cleared to 0xFFFFFFFF, so the order of the writes cannot matter.  Texels outside the atlas are never written.
 *
 *   Eviction.  After the ownership of a stage, every face of the stage's charts that covers a centre whose owner is another face
 *   is EVICTED (evicted[f] = 1, every other face 0); then every texel whose owner is an evicted face becomes unowned.  The faces
 *   that remain own disjoint sets of centres.  Stage 0 labels the classified faces, stage 1 the faces evicted in stage 0 (their
 *   charts packed below at the same W), stage 2 makes every face evicted in stage 1 a chart of its own, packed below in face
 *   order; a single triangle cannot overlap itself.
 *
 *   Dilation.  pad passes, each reading the previous pass's map: an unowned texel takes the owner of the first owned neighbour in
 *   the order (x-1,y) (x+1,y) (x,y-1) (x,y+1) (x-1,y-1) (x+1,y-1) (x-1,y+1) (x+1,y+1); neighbours outside the atlas are skipped.
 *   Owned centres lie at least pad texels inside their rectangle, so no border reaches another rectangle.  The result read as
 *   int32 is texel_face (H, W), -1 where nothing reached.
 *
 *   Texel point.  The face's atlas corners a, b, c are read from corner_texels (UVs, below), so that the points stay those of the
 *   atlas when the vertices move later; area = E_ab(c) in int64 (the wrapped product for corners no atlas has).  A texel with f =
 *   texel_face outside [0, n_faces), a face with an index out of range or area <= 0 (a face without a chart has zero corners) is
 *   INVALID.  Otherwise, with the centre P:
 *     beta  = (float)((double)E_ca(P) / (double)area),   gamma = (float)((double)E_ab(P) / (double)area)
 *     p_k = (a_k + beta * (b_k - a_k)) + gamma * (c_k - a_k)                  (f32, the world vertices)
 *   outside [0, 1] on a dilated texel these extrapolate the face's plane.  If a p_k is not finite the texel is INVALID;
 *   otherwise point_k = min(max(p_k, box_lo_k), box_hi_k).  With the vertex normals na, nb, nc:
 *     n_k = (na_k + beta * (nb_k - na_k)) + gamma * (nc_k - na_k),  L = sqrt((n_0 n_0 + n_1 n_1) + n_2 n_2),  dir_k = -(n_k / L)
 *   and (0, 0, 1) if L is not > 0 or a dir_k is not finite.  Invalid texels get point = box_lo, dir = (0, 0, 1), valid = 0.
 *
 *   UVs.  corner_texels (n_faces, 3, 2) i32: the atlas coordinates (x, y) in sixteenths of every corner; zeros for a face of
 *   class 6 or with a face_chart outside [0, n_charts).  uvs (n_faces, 3, 2) f32, each f64 expression rounded once:
 *     u = (float)(((double)x / 16.0) / (double)W),   v = (float)(1.0 - ((double)y / 16.0) / (double)H)
 *   OBJ's bottom-left origin.  Inside a chart a vertex has one UV.
 *
 *   Render.  Projection, key buffer and the winner's clamped perspective-correct weights beta, gamma are exactly those of
 *   csrc/meshatlas/ngp_meshatlas.h (the shared rasteriser).  With c* = (float)corner_texels / 16.0f of the winning face:
 *     X = ((ca_x + beta * (cb_x - ca_x)) + gamma * (cc_x - ca_x)) - 0.5f,   Y likewise
 *   texel i has its centre at X = i, and the bilinear lookup with its clamps is that header's: every read stays inside the atlas
 *   whatever corner_texels holds.
 *
 * Labels are minima and the ownership map takes minima, so all outputs but the order inside vf_faces are bit-identical run to
 * run, for any launch shape and any split of the texels or cameras into chunks.  No kernel reads or writes through an
 * out-of-range index, a bad face or a NaN vertex.
 */
#ifndef NGP_MESHCHART_H
#define NGP_MESHCHART_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef NGP_EINVAL
#define NGP_EINVAL   (-1)  /* bad argument (null pointer, negative size, size out of range, workspace too small, not finite) */
#endif
#ifndef NGP_ERANGE
#define NGP_ERANGE   (-5)  /* more than INT32_MAX vertices, faces or cameras, or an atlas wider or higher than 16384 texels */
#endif

#define NGP_MESHCHART_NO_CLASS 6
#define NGP_MESHCHART_MAX_PAD 8

/* ABI version of this library (1). */
int ngp_meshchart_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshchart_build_arch(void);

/* Bytes of workspace ngp_meshchart_classify needs (a multiple of 256, never 0 for sizes in range); 0 if n_vertices is outside
 * [0, INT32_MAX] or n_faces outside [1, INT32_MAX]. */
size_t ngp_meshchart_classify_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* face_class (n_faces) u8, vf_offsets (n_vertices + 1) i64 and vf_faces (3 n_faces) i32 (THE RULE: Snap, Class, Vertex table).
 * workspace: device, 8-byte aligned.  n_vertices may be 0 (vertices may then be NULL): every face then has class 6. */
int ngp_meshchart_classify(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float texel_size,
                           uint8_t* face_class, int64_t* vf_offsets, int32_t* vf_faces, void* workspace, size_t workspace_bytes,
                           void* stream);

/* Bytes of workspace ngp_meshchart_label needs; 0 if n_faces is outside [1, INT32_MAX]. */
size_t ngp_meshchart_label_workspace_bytes(int64_t n_faces);

/* The charts of one stage (THE RULE: Charts of a stage): face_label (n_faces) i32, face_chart (n_faces) i32 (active faces only)
 * and n_charts (1) i64 ON THE DEVICE, the number of charts of the stage.  active (n_faces) u8; face_class, vf_offsets and
 * vf_faces are ngp_meshchart_classify's.  chart_base >= 0.  workspace: device, 8-byte aligned. */
int ngp_meshchart_label(const int32_t* faces, int64_t n_vertices, int64_t n_faces, const uint8_t* face_class, const uint8_t* active,
                        const int64_t* vf_offsets, const int32_t* vf_faces, int unite, int64_t chart_base, int32_t* face_label,
                        int32_t* face_chart, int64_t* n_charts, void* workspace, size_t workspace_bytes, void* stream);

/* chart_bounds (chart_hi - chart_lo, 4) i32: umin, vmin, umax, vmax in sixteenths of the charts chart_lo .. chart_hi - 1 (THE
 * RULE: Bounds of a chart); INT32_MAX and INT32_MIN for a chart without a face.  0 <= chart_lo < chart_hi <= INT32_MAX. */
int ngp_meshchart_bounds(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float texel_size,
                         const int32_t* face_chart, int64_t chart_lo, int64_t chart_hi, int32_t* chart_bounds, void* stream);

/* THE RULE's packing of n HOST rectangles sizes (n, 2) i32 = (w, h), each in [1, 16384]: origins (n, 2) HOST i32 = (x, y), order
 * (n) HOST i32 (the order they were placed in), the atlas width and the height so far.  Host only: nothing is launched.
 * width_in == 0 chooses the width (y0 must then be 0); otherwise 1 <= width_in <= 16384, 0 <= y0 <= 16384 and no rectangle may
 * be wider than width_in (NGP_EINVAL).  NGP_ERANGE when the atlas would be wider or higher than 16384 texels. */
int ngp_meshchart_pack(const int32_t* sizes, int64_t n, int sorted, int width_in, int y0, int32_t* origins, int32_t* order, int* width,
                       int* height);

/* The owners of the texel centres that the faces of the charts chart_lo .. chart_hi - 1 cover (THE RULE: Ownership), by atomic
 * minimum into owner (height, width) u32, which the caller cleared to 0xFFFFFFFF where nothing is owned yet.  chart_rects
 * (n_charts, 6) i32; 0 <= chart_lo <= chart_hi <= n_charts; width and height in [1, 16384]; 0 <= pad <= 8. */
int ngp_meshchart_raster(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float texel_size,
                         const int32_t* face_chart, const int32_t* chart_rects, int64_t n_charts, int64_t chart_lo, int64_t chart_hi,
                         int pad, int width, int height, uint32_t* owner, void* stream);

/* THE RULE's eviction after ngp_meshchart_raster with the same arguments: evicted (n_faces) u8, n_evicted (1) i64 ON THE DEVICE,
 * and the texels of evicted faces cleared in owner. */
int ngp_meshchart_evict(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float texel_size,
                        const int32_t* face_chart, const int32_t* chart_rects, int64_t n_charts, int64_t chart_lo, int64_t chart_hi,
                        int pad, int width, int height, uint32_t* owner, uint8_t* evicted, int64_t* n_evicted, void* stream);

/* pad passes of THE RULE's dilation over owner (height, width) u32 with scratch of the same size; the result is left in owner. */
int ngp_meshchart_dilate(uint32_t* owner, uint32_t* scratch, int width, int height, int pad, void* stream);

/* corner_texels (n_faces, 3, 2) i32 and uvs (n_faces, 3, 2) f32 (THE RULE: UVs). */
int ngp_meshchart_corners(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float texel_size,
                          const int32_t* face_chart, const int32_t* chart_rects, int64_t n_charts, int pad, int width, int height,
                          int32_t* corner_texels, float* uvs, void* stream);

/* points (count, 3) f32, dirs (count, 3) f32 and valid (count) u8 of the texels begin .. begin + count - 1 of the row-major
 * atlas texel_face (height, width) i32 with the faces' corner_texels (n_faces, 3, 2) i32: the caller chunks, and the result does not depend on the chunks.  begin >= 0, count >=
 * 0, begin + count <= width * height; with count == 0 nothing is launched and the device pointers are not looked at. */
int ngp_meshchart_texel_points(const float* vertices, const int32_t* faces, const float* normals, int64_t n_vertices, int64_t n_faces,
                               const int32_t* corner_texels, int width, int height, const int32_t* texel_face, const float* box,
                               int64_t begin, int64_t count, float* points, float* dirs, uint8_t* valid, void* stream);

/* Bytes of n_cams key buffers of W x H pixels: 8 * W * H * n_cams.  0 if W or H is outside [1, 16384] or n_cams outside
 * [1, INT32_MAX].  ngp_meshchart_render accepts any workspace that holds at least one camera. */
size_t ngp_meshchart_render_workspace_bytes(int W, int H, int64_t n_cams);

/* image (n_cams, H, W, 3) f32, face_index (n_cams, H, W) i32 or NULL, depth (n_cams, H, W) f32 or NULL: the mesh with its texture
 * (atlas_height, atlas_width, 3) u8, each in [1, 16384], and its corner_texels seen from every camera (THE RULE, Render).
 * workspace: device, 8-byte aligned, room for at least one camera (8 * W * H bytes); the cameras are processed in chunks of as
 * many as fit.  near_distance finite; background: three finite HOST floats.  n_vertices may be 0: every pixel is background. */
int ngp_meshchart_render(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, const int32_t* corner_texels,
                         const uint8_t* texture, int atlas_width, int atlas_height, const float* K, const float* poses, int64_t n_cams,
                         int W, int H, float near_distance, const float* background, void* workspace, size_t workspace_bytes,
                         float* image, int32_t* face_index, float* depth, void* stream);

#ifdef __cplusplus
}
#endif

#endif
