/*
 * ngp_meshtex.h -- C ABI of libngp_meshtex.so: a texture atlas for an indexed triangle mesh (layout, the world point and viewing
 * direction of every texel, the faces' UV coordinates) and a renderer of the textured mesh against pinhole cameras, on gfx950.
 *
 * A library of its own beside libngp_hip.so (include/ngp_hip.h), libngp_mesh.so (include/ngp_mesh.h), libngp_meshfilter.so
 * (include/ngp_meshfilter.h), libngp_meshcull.so (include/ngp_meshcull.h), libngp_meshsimplify.so (include/ngp_meshsimplify.h),
 * libngp_meshtsdf.so (include/ngp_meshtsdf.h) and libngp_meshsmooth.so (include/ngp_meshsmooth.h), with their conventions: raw
 * DEVICE pointers, caller-allocated outputs and workspace, the hipStream_t passed as void*, 0 on success, a positive hipError_t if
 * a launch failed, a negative NGP_E* code for bad arguments.  No entry point allocates or synchronises, and every argument is
 * checked on the host before anything is launched.  This header needs none of the other seven and may be included before or
 * after them.
 *
 * Mesh: vertices (n_vertices, 3) f32 in world coordinates, faces (n_faces, 3) i32, normals (n_vertices, 3) f32.  Cameras: poses
 * (n_cams, 3, 4) f32 row-major camera-to-world [R | t], K (3, 3) f32 row-major, images of W x H pixels: the conventions of
 * include/ngp_meshcull.h.  box: six HOST floats lo0 lo1 lo2 hi0 hi1 hi2, finite, lo <= hi.  background: three HOST floats.
 *
 * THE RULE.  f32 operations are IEEE binary32, one rounding each, in the order written, left to right, no fused multiply-add;
 * divisions and square roots are correctly rounded; floor() is the f32 floor; min and max are only ever applied to
 * numbers that are not NaN.
 *
 *   Atlas layout.  T = texels, the texel intervals along a face's leg, 1 <= T <= 256.  A cell is CW = T + 5 texels wide and
 *   CH = T + 4 texels high and holds two faces: face f lies in cell g = f >> 1, slot s = f & 1.  n_cells = ceil(n_faces / 2).
 *   cells_per_row is the smallest c >= 1 with c * CW >= ceil(n_cells / c) * CH; W = c * CW, H = ceil(n_cells / c) * CH.  If W or
 *   H exceeds 16384 the call returns NGP_ERANGE.  Cell g has its origin at texel (ox, oy) = ((g % c) * CW, (g / c) * CH).  The
 *   atlas is row-major, texel (x, y) is element y * W + x, and image row 0 is the top row.
 *
 *   Texel ownership.  A texel (i, j) local to its cell belongs to slot 0 when i + j <= T + 3; its slot coordinates are then
 *   (i', j') = (i, j).  Otherwise it belongs to slot 1 with (i', j') = (T + 4 - i, T + 3 - j).  The two slots tile the cell
 *   exactly, half each.  A texel whose slot has no face (the odd last face's partner, the cells past n_cells) is INVALID, and so
 *   is a texel whose face has an index outside [0, n_vertices): nothing is read through such an index.
 *
 *   Face corners.  The corners a, b, c of a face sit at the slot coordinates (1, 1), (1 + T, 1) and (1, 1 + T), which are texel
 *   centres.  A one-texel extrapolated border then surrounds every face, so a bilinear lookup inside a face only gives weight to
 *   texels the face owns.
 *
 *   Texel point.  For a texel that is not invalid so far, with the face's vertices a, b, c:
 *     u = (float)(i' - 1) / (float)T,  v = (float)(j' - 1) / (float)T
 *     p_k = (a_k + u * (b_k - a_k)) + v * (c_k - a_k)
 *   If a p_k is not finite the texel is INVALID.  Otherwise point_k = min(max(p_k, box_lo_k), box_hi_k): a border texel of a
 *   face at the box's edge would otherwise leave the box.
 *
 *   Texel direction.  With the vertex normals na, nb, nc of the face's corners:
 *     n_k   = (na_k + u * (nb_k - na_k)) + v * (nc_k - na_k)
 *     L     = sqrt((n_0 * n_0 + n_1 * n_1) + n_2 * n_2)
 *     dir_k = -(n_k / L)
 *   If L is not > 0 (NaN included), or a dir_k is not finite, the direction is (0, 0, 1).
 *   Invalid texels get point = box_lo, dir = (0, 0, 1), valid = 0; every other texel valid = 1.
 *
 *   UVs.  A corner at atlas texel (gi, gj) -- (ox + i, oy + j) of its local texel -- has, in f64 rounded once to f32,
 *     u = (float)(((double)gi + 0.5) / (double)W)
 *     v = (float)(1.0 - ((double)gj + 0.5) / (double)H)
 *   which is OBJ's bottom-left origin.  Every face gets UVs, whatever its indices.
 *
 *   Render: projection and key buffer.  Projection (m, s, p, ud, vd, d, u, v, q = 1 / d), the face conditions (indices inside
 *   [0, n_vertices), all three d >= near, area non-zero and finite), the pixel box, the edge functions E_ab, E_bc, E_ca, the
 *   pixel centre P = (i + 0.5, j + 0.5), w_a = E_bc(P), w_b = E_ca(P), w_c = E_ab(P), the coverage test (inclusive edges, either
 *   winding) and
 *     z = area / (w_a * q_a + w_b * q_b + w_c * q_c)          (z finite and > 0, otherwise dropped)
 *   are exactly those of include/ngp_meshcull.h.  Per pixel the buffer holds the MINIMUM over the faces that cover it of the
 *   64-bit key (bits(z) << 32) | face index, taken by an unsigned 64-bit atomic minimum from a buffer cleared to all ones: the
 *   nearest face wins, and at bit-equal depth the smaller index.
 *
 *   Render: shading a pixel that holds a key.  Recompute w_a, w_b, w_c and q_a, q_b, q_c of the winning face f at the pixel
 *   centre, as the raster did.  With (ox, oy) the origin of f's cell:
 *     l_a = w_a * q_a,  l_b = w_b * q_b,  l_c = w_c * q_c
 *     sum = (l_a + l_b) + l_c
 *     beta  = min(max(l_b / sum, 0), 1)
 *     gamma = min(max(l_c / sum, 0), 1)
 *     x' = 1 + beta * (float)T,  y' = 1 + gamma * (float)T
 *     slot 0:  X = (float)ox + x',                       Y = (float)oy + y'
 *     slot 1:  X = (float)ox + ((float)(T + 4) - x'),    Y = (float)oy + ((float)(T + 3) - y')
 *   Texel i has its centre at X = i.
 *     i0 = (int)floor(X),  fx = X - floor(X),  i1 = min(i0 + 1, W_atlas - 1);  j0, fy, j1 likewise from Y and H_atlas
 *   and per channel, with t = (float)byte of the texture at (column, row):
 *     top    = t(i0, j0) * (1 - fx) + t(i1, j0) * fx
 *     bot    = t(i0, j1) * (1 - fx) + t(i1, j1) * fx
 *     colour = (top * (1 - fy) + bot * fy) / 255
 *   depth is z and face_index is f, both from the key.  A pixel without a key gets the background colour, face index -1 and
 *   depth +inf.
 *
 * Every texel and every pixel is a single expression of the inputs and the key buffer takes a minimum, which does not depend on
 * the order of the writes: all outputs are bit-identical run to run, for any launch shape and for any split of the texels or the
 * cameras into chunks.  No kernel reads or writes through an out-of-range index, a bad face or a NaN vertex.
 */
#ifndef NGP_MESHTEX_H
#define NGP_MESHTEX_H

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

/* ABI version of this library (1). */
int ngp_meshtex_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshtex_build_arch(void);

/* The atlas layout of THE RULE for n_faces >= 1 faces at `texels` = T in [1, 256]: cells per row, width and height in texels.
 * Host only: nothing is launched.  NGP_EINVAL for a null pointer, n_faces < 1 or T out of range; NGP_ERANGE when n_faces exceeds
 * INT32_MAX or the atlas would be wider or higher than 16384 texels (nothing is written then). */
int ngp_meshtex_atlas_size(int64_t n_faces, int texels, int* cells_per_row, int* width, int* height);

/* points (count, 3) f32, dirs (count, 3) f32 and valid (count) u8 of the texels begin .. begin + count - 1 of the row-major
 * atlas: the caller chunks, and the result does not depend on the chunks.  The layout is recomputed inside from n_faces and
 * texels.  box: six HOST floats (above).  begin >= 0, count >= 0, begin + count <= width * height; with count == 0 nothing is
 * launched and the device pointers are not looked at.  n_vertices may be 0 (vertices and normals may then be NULL): every texel is then invalid. */
int ngp_meshtex_texel_points(const float* vertices, const int32_t* faces, const float* normals, int64_t n_vertices, int64_t n_faces,
                             int texels, const float* box, int64_t begin, int64_t count, float* points, float* dirs, uint8_t* valid,
                             void* stream);

/* uvs (n_faces, 3, 2) f32: u, v of the corners a, b, c of every face (THE RULE, UVs). */
int ngp_meshtex_face_uvs(int64_t n_faces, int texels, float* uvs, void* stream);

/* Bytes of n_cams key buffers of W x H pixels: 8 * W * H * n_cams.  0 if W or H is outside [1, 16384] or n_cams outside
 * [1, INT32_MAX].  ngp_meshtex_render accepts any workspace that holds at least one camera. */
size_t ngp_meshtex_render_workspace_bytes(int W, int H, int64_t n_cams);

/* image (n_cams, H, W, 3) f32, face_index (n_cams, H, W) i32 or NULL, depth (n_cams, H, W) f32 or NULL: the mesh with its texture
 * (H_atlas, W_atlas, 3) u8 -- the atlas of n_faces and texels -- seen from every camera (THE RULE, Render).  workspace: device,
 * 8-byte aligned, workspace_bytes of it, room for at least one camera (8 * W * H bytes); the cameras are processed in chunks of as
 * many as fit: per chunk the keys are cleared, the faces are rasterised and the pixels are shaded.  near_distance is the rule's
 * `near` (finite); background: three finite HOST floats.  W and H run from 1 to 16384, n_cams >= 1, n_faces >= 1; n_vertices may be 0 (vertices may then be
 * NULL): every pixel is then background. */
int ngp_meshtex_render(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, int texels,
                       const uint8_t* texture, const float* K, const float* poses, int64_t n_cams, int W, int H, float near_distance,
                       const float* background, void* workspace, size_t workspace_bytes, float* image, int32_t* face_index,
                       float* depth, void* stream);

#ifdef __cplusplus
}
#endif

#endif
