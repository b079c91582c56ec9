/*
 * ngp_meshatlas.h -- C ABI of libngp_meshatlas.so: a texture atlas whose texel density follows the size of every face (a class
 * of texel intervals per face from its longest edge, the faces sorted by class, one band of cells per class, the world point and
 * viewing direction of every texel, the faces' UV coordinates) and a renderer of the mesh textured that way, on gfx950.
 *
 * A library of its own beside the other twelve (include/ngp_hip.h, ngp_mesh.h, ngp_meshfilter.h, ngp_meshcull.h,
 * ngp_meshsimplify.h, ngp_meshtsdf.h, ngp_meshsmooth.h, ngp_meshtex.h, ngp_metrics.h, ngp_meshdist.h, ngp_meshquadric.h,
 * ngp_meshdecimate.h), with their conventions: raw DEVICE pointers, caller-allocated outputs and workspace, the hipStream_t
 * passed as void*, 0 on success, a positive hipError_t if a launch failed, a negative NGP_E* code for bad arguments.  No entry
 * point allocates or synchronises, and every argument is checked on the host before anything is launched.  This header needs
 * none of the others and may be included before or after them.  It lies beside the library's sources, not under include/.  libngp_meshtex.so (the atlas with the same texels for every
 * face) is not changed and not needed.
 *
 * Mesh: vertices (n_vertices, 3) f32 in world coordinates, faces (n_faces, 3) i32, normals (n_vertices, 3) f32.  Cameras: poses
 * (n_cams, 3, 4) f32 row-major camera-to-world [R | t], K (3, 3) f32 row-major, images of W x H pixels: the conventions of
 * include/ngp_meshcull.h.  box: six HOST floats lo0 lo1 lo2 hi0 hi1 hi2, finite, lo <= hi.  background: three HOST floats.
 * counts: sixteen HOST int64, the class sizes that ngp_meshatlas_classify wrote to the device and the caller read back (128
 * bytes, the one host read of the pipeline): each >= 0, their sum n_faces.
 *
 * THE RULE.  f32 operations are IEEE binary32, one rounding each, in the order written, left to right, no fused multiply-add;
 * divisions and square roots are correctly rounded; floor() is the f32 floor; min and max are only ever applied to numbers
 * that are not NaN.
 *
 *   Ladder.  Sixteen classes c = 0..15 with T_c = 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256 texel intervals
 *   along a face's leg: half-octave steps.
 *
 *   Class of a face.  texel_size = s (f32, finite, > 0: world units per texel interval), 0 <= cmin <= cmax <= 15.  A face with
 *   an index outside [0, n_vertices) has class cmin; nothing is read through such an index.  Otherwise, for each edge from p to q
 *   (ab: a to b, bc: b to c, ca: c to a):
 *     d_k = q_k - p_k,  e = (d_0 * d_0 + d_1 * d_1) + d_2 * d_2
 *     m = e_ab;  if (e_bc > m) m = e_bc;  if (e_ca > m) m = e_ca
 *   If m is not finite the class is cmin.  Otherwise it is the smallest c in [cmin, cmax] with m <= t * t, t = (float)T_c * s,
 *   and cmax if there is none: no edge of a face is sampled coarser than s unless cmax caps it.
 *
 *   Order.  order[r] = f lists the faces by class DESCENDING and, inside a class, by face index ascending (a stable counting
 *   sort of one digit).  count[c] is the number of faces of class c and base[c] = sum of count[c'] over c' > c.
 *
 *   Layout, a function of count[16] alone.  Class c with count[c] > 0 uses the cell of include/ngp_meshtex.h with T = T_c: CW =
 *   T + 5 texels wide, CH = T + 4 texels high, two faces per cell.  For an atlas width W:
 *     cpr_c = floor(W / CW_c),  cells_c = ceil(count[c] / 2),  rows_c = ceil(cells_c / cpr_c),  h_c = rows_c * CH_c
 *   The bands are stacked from row 0 downwards, the largest class first: y_c = sum of h_c' over non-empty c' > c, and H(W) = sum
 *   of h_c.  W is the smallest integer >= CW of the largest non-empty class with H(W) <= W (H does not increase with W), and
 *   H = H(W).  If W would exceed 16384 the call returns NGP_ERANGE.  The face of rank r in class c has q = r - base[c], cell
 *   g = q >> 1, slot q & 1, and its cell has its origin at texel (ox, oy) = ((g % cpr_c) * CW_c, y_c + (g / cpr_c) * CH_c).
 *   The atlas is row-major, texel (x, y) is element y * W + x, and image row 0 is the top row.
 *
 *   Face record.  face_place (n_faces, 2) i32:  [0] = ox | oy << 16,  [1] = c | slot << 8.
 *
 *   Texel ownership inside a cell, with T = T_c.  A texel (i, j) local to its cell belongs to slot 0 when i + j <= T + 3; its
 *   slot coordinates are then (i', j') = (i, j).  Otherwise it belongs to slot 1 with (i', j') = (T + 4 - i, T + 3 - j).  The
 *   corners a, b, c of a face sit at the slot coordinates (1, 1), (1 + T, 1) and (1, 1 + T): a one-texel extrapolated border
 *   surrounds every face, so a bilinear lookup inside a face only gives weight to texels the face owns.
 *
 *   Texel -> face.  Texel (x, y) lies in the band c with y_c <= y < y_c + h_c; row = (y - y_c) / CH_c and j the remainder, col =
 *   x / CW_c and i the remainder.  With g = row * cpr_c + col and q = 2 g + slot: col >= cpr_c (the right margin), g >= cells_c
 *   or q >= count[c] makes the texel INVALID.  Otherwise f = order[base[c] + q]; f outside [0, n_faces) or a face with an index
 *   outside [0, n_vertices) makes the texel INVALID as well, and nothing is read through such an index.
 *
 *   Texel point.  For a texel that is not invalid so far, with the face's vertices a, b, c and T = T_c:
 *     u = (float)(i' - 1) / (float)T,  v = (float)(j' - 1) / (float)T
 *     p_k = (a_k + u * (b_k - a_k)) + v * (c_k - a_k)
 *   If a p_k is not finite the texel is INVALID.  Otherwise point_k = min(max(p_k, box_lo_k), box_hi_k).
 *
 *   Texel direction.  With the vertex normals na, nb, nc of the face's corners:
 *     n_k   = (na_k + u * (nb_k - na_k)) + v * (nc_k - na_k)
 *     L     = sqrt((n_0 * n_0 + n_1 * n_1) + n_2 * n_2)
 *     dir_k = -(n_k / L)
 *   If L is not > 0 (NaN included), or a dir_k is not finite, the direction is (0, 0, 1).
 *   Invalid texels get point = box_lo, dir = (0, 0, 1), valid = 0; every other texel valid = 1.
 *
 *   UVs.  From face_place: ox = [0] & 0xFFFF, oy = ([0] >> 16) & 0xFFFF, c = [1] & 15, slot = ([1] >> 8) & 1, T = T_c.  The
 *   corner at slot coordinates (i', j') is the atlas texel (gi, gj) = (ox + i', oy + j') in slot 0 and (ox + T + 4 - i',
 *   oy + T + 3 - j') in slot 1, and in f64 rounded once to f32
 *     u = (float)(((double)gi + 0.5) / (double)W)
 *     v = (float)(1.0 - ((double)gj + 0.5) / (double)H)
 *   which is OBJ's bottom-left origin.  Every face gets UVs, whatever its indices.
 *
 *   Render: projection and key buffer.  Projection (m, s, p, ud, vd, d, u, v, q = 1 / d), the face conditions (indices inside
 *   [0, n_vertices), all three d >= near, area non-zero and finite), the pixel box, the edge functions E_ab, E_bc, E_ca, the
 *   pixel centre P = (i + 0.5, j + 0.5), w_a = E_bc(P), w_b = E_ca(P), w_c = E_ab(P), the coverage test (inclusive edges, either
 *   winding) and
 *     z = area / (w_a * q_a + w_b * q_b + w_c * q_c)          (z finite and > 0, otherwise dropped)
 *   are exactly those of include/ngp_meshcull.h and include/ngp_meshtex.h.  Per pixel the buffer holds the MINIMUM over the
 *   faces that cover it of the 64-bit key (bits(z) << 32) | face index, taken by an unsigned 64-bit atomic minimum from a buffer
 *   cleared to all ones: the nearest face wins, and at bit-equal depth the smaller index.
 *
 *   Render: shading a pixel that holds a key.  Recompute w_a, w_b, w_c and q_a, q_b, q_c of the winning face f at the pixel
 *   centre, as the raster did.  ox, oy, c, slot and T = T_c come from face_place[f] by the masks written under UVs, whatever the
 *   record holds:
 *     l_a = w_a * q_a,  l_b = w_b * q_b,  l_c = w_c * q_c
 *     sum = (l_a + l_b) + l_c
 *     beta  = min(max(l_b / sum, 0), 1)
 *     gamma = min(max(l_c / sum, 0), 1)
 *     x' = 1 + beta * (float)T,  y' = 1 + gamma * (float)T
 *     slot 0:  X = (float)ox + x',                       Y = (float)oy + y'
 *     slot 1:  X = (float)ox + ((float)(T + 4) - x'),    Y = (float)oy + ((float)(T + 3) - y')
 *   Texel i has its centre at X = i.
 *     i0 = min(max((int)floor(X), 0), W_atlas - 1),  fx = X - floor(X),  i1 = min(i0 + 1, W_atlas - 1)
 *     j0, fy, j1 likewise from Y and H_atlas
 *   so the four texels lie inside the atlas whatever face_place holds (for a record of THE RULE the clamps change nothing), and
 *   per channel, with t = (float)byte of the texture at (column, row):
 *     top    = t(i0, j0) * (1 - fx) + t(i1, j0) * fx
 *     bot    = t(i0, j1) * (1 - fx) + t(i1, j1) * fx
 *     colour = (top * (1 - fy) + bot * fy) / 255
 *   depth is z and face_index is f, both from the key.  A pixel without a key gets the background colour, face index -1 and
 *   depth +inf.
 *
 * The sort takes every position from counts (ballots within a wave, sums over waves and blocks): no atomic operation decides a
 * position.  Every texel and every pixel is a single expression of the inputs and the key buffer takes a minimum, which does not
 * depend on the order of the writes: all outputs are bit-identical run to run, for any launch shape and for any split of the
 * texels or the cameras into chunks.  No kernel reads or writes through an out-of-range index, a bad face or a NaN vertex.
 */
#ifndef NGP_MESHATLAS_H
#define NGP_MESHATLAS_H

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

#define NGP_MESHATLAS_CLASSES 16

/* ABI version of this library (1). */
int ngp_meshatlas_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshatlas_build_arch(void);

/* Bytes of workspace ngp_meshatlas_classify needs for n_faces faces (a multiple of 256, never 0 for a size in range); 0 if
 * n_faces is outside [1, INT32_MAX]. */
size_t ngp_meshatlas_classify_workspace_bytes(int64_t n_faces);

/* face_class (n_faces) u8, order (n_faces) i32 and counts (16) i64 ON THE DEVICE (THE RULE: Class of a face, Order).  workspace:
 * device, 8-byte aligned, at least ngp_meshatlas_classify_workspace_bytes(n_faces) bytes.  n_faces >= 1; n_vertices may be 0
 * (vertices may then be NULL): every face then has class cmin. */
int ngp_meshatlas_classify(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float texel_size, int cmin,
                           int cmax, uint8_t* face_class, int32_t* order, int64_t* counts, void* workspace, size_t workspace_bytes,
                           void* stream);

/* The layout of THE RULE for the HOST counts: atlas width and height in texels and, when bands is not NULL, bands (16, 4) HOST
 * i32 with y_c, h_c, cpr_c, cells_c per class (all 0 for an empty class).  Host only: nothing is launched.  NGP_EINVAL for a
 * null pointer, a negative count or no face at all; NGP_ERANGE when the counts sum to more than INT32_MAX or the atlas would be
 * wider than 16384 texels (nothing is written then). */
int ngp_meshatlas_layout(const int64_t* counts, int* width, int* height, int32_t* bands);

/* face_place (n_faces, 2) i32 of THE RULE (Face record) from the device's order and the HOST counts, which must sum to n_faces.
 * An order[r] outside [0, n_faces) writes nothing. */
int ngp_meshatlas_place(const int32_t* order, const int64_t* counts, int64_t n_faces, int32_t* face_place, void* stream);

/* points (count, 3) f32, dirs (count, 3) f32 and valid (count) u8 of the texels begin .. begin + count - 1 of the row-major
 * atlas: the caller chunks, and the result does not depend on the chunks.  The layout is recomputed inside from the HOST counts
 * (their sum n_faces).  begin >= 0, count >= 0, begin + count <= width * height; with count == 0 nothing is launched and the
 * device pointers are not looked at.  n_vertices may be 0 (vertices and normals may then be NULL): every texel is then invalid. */
int ngp_meshatlas_texel_points(const float* vertices, const int32_t* faces, const float* normals, int64_t n_vertices, int64_t n_faces,
                               const int32_t* order, const int64_t* counts, const float* box, int64_t begin, int64_t count,
                               float* points, float* dirs, uint8_t* valid, void* stream);

/* uvs (n_faces, 3, 2) f32: u, v of the corners a, b, c of every face (THE RULE, UVs) in an atlas of width x height texels, each
 * in [1, 16384]. */
int ngp_meshatlas_face_uvs(const int32_t* face_place, int64_t n_faces, int width, int height, float* uvs, void* stream);

/* Bytes of n_cams key buffers of W x H pixels: 8 * W * H * n_cams.  0 if W or H is outside [1, 16384] or n_cams outside
 * [1, INT32_MAX].  ngp_meshatlas_render accepts any workspace that holds at least one camera. */
size_t ngp_meshatlas_render_workspace_bytes(int W, int H, int64_t n_cams);

/* image (n_cams, H, W, 3) f32, face_index (n_cams, H, W) i32 or NULL, depth (n_cams, H, W) f32 or NULL: the mesh with its texture
 * (atlas_height, atlas_width, 3) u8, each in [1, 16384], and its face_place seen from every camera (THE RULE, Render).
 * workspace: device, 8-byte aligned, workspace_bytes of it, room for at least one camera (8 * W * H bytes); the cameras are
 * processed in chunks of as many as fit.  near_distance is the rule's `near` (finite); background: three finite HOST floats.
 * W and H run from 1 to 16384, n_cams >= 1, n_faces >= 1; n_vertices may be 0 (vertices may then be NULL): every pixel is then
 * background. */
int ngp_meshatlas_render(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, const int32_t* face_place,
                         const uint8_t* texture, int atlas_width, int atlas_height, const float* K, const float* poses, int64_t n_cams,
                         int W, int H, float near_distance, const float* background, void* workspace, size_t workspace_bytes,
                         float* image, int32_t* face_index, float* depth, void* stream);

#ifdef __cplusplus
}
#endif

#endif
