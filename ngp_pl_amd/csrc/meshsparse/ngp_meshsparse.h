/*
 * ngp_meshsparse.h -- C ABI of libngp_meshsparse.so: marching cubes over the 8^3-point bricks of the export lattice that touch
 * occupied cells of the occupancy grid, instead of over a dense volume, on gfx950.
 *
 * A library of its own beside the others, with their conventions: raw DEVICE pointers, caller-allocated outputs and workspace,
 * the hipStream_t passed as void*, 0 on success, a positive hipError_t if a launch failed, a negative NGP_E* code for bad
 * arguments.  No entry point allocates or synchronises, and every argument is checked on the host before anything is launched.
 * This header needs none of the others and may be included before or after them.  It lies beside the library's sources, not
 * under include/.  No other library is changed or needed.
 *
 * THE CONTRACT.
 *
 *   Lattice.  The lattice of nx x ny x nz points, its linear index (k*ny + j)*nx + i, the point positions lo + (i, j, k) * h with
 *   h = (hi - lo) / (n - 1) in f32 per axis, the inside rule (sigma > threshold), vertices, normals, face orientation and table
 *   order are exactly those of include/ngp_mesh.h.  bounds6 is a HOST pointer to {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z}.
 *
 *   Bricks.  nb = (n + 7) / 8 per axis.  Brick (bx, by, bz) owns the lattice points 8b .. min(8b + 7, n - 1) per axis and the
 *   cells whose lowest corner is one of those points; it has the number (bz*nby + by)*nbx + bx.  A point of a brick has the local
 *   index ((k & 7)*8 + (j & 7))*8 + (i & 7).  Each axis may have 2..65535 points and the grid at most 2^30 bricks: outside that
 *   the workspace queries return 0 and the calls NGP_EINVAL.
 *
 *   Masks.  A mesh mask is one byte per brick (0: not meshed), in brick order.  The sample mask is its dilation by the 26
 *   neighbours, clipped to the grid.  Every corner of every cell of a meshed brick, and every point the central differences of the
 *   normals of those cells' vertices read (they reach -1 and +2 along an edge), then lies in a sampled brick.  At the border of
 *   the LATTICE the differences are one-sided, as in the dense extractor.
 *
 *   Slots and the pool.  The sampled bricks in ascending brick number are the sample slots 0, 1, ...; brick_table (one int32 per
 *   brick) holds a brick's sample slot, -1 for a brick that is not sampled; sample_bricks and mesh_bricks list the brick numbers of
 *   the sampled and of the meshed bricks, ascending.  The pool holds 512 f32 per sample slot, sigma of the brick's points by local
 *   index.  Slots of a partial brick past the lattice's end are never read.
 *
 *   Result.  The faces of the dense mesh whose cell belongs to a meshed brick, and exactly the vertices those faces reference,
 *   each once.  Positions and normals have the dense extractor's bits on the same sigma values.  vertex_key[v] is
 *   3 * (linear index of the owning point) + axis; face_cell[f] is the linear index of the cell's lowest corner.  Raw order:
 *   vertices by the owning point's brick in ascending brick number, then local index, then axis; faces by the cell's brick in
 *   ascending brick number, then local index, then table order.  No atomic operation takes part in it: the result is bit-identical
 *   from run to run.  Sorting the vertices by key and the faces stably by face_cell gives the dense numbering restricted to the
 *   meshed cells.
 *
 *   Mask from the occupancy grid (ngp_meshsparse_mask).  All arithmetic is IEEE binary64, one rounding per operation, in the order
 *   written, no fused multiply-add.  Per axis, with lo, hi the f32 bounds widened to f64:
 *     h = (hi - lo) / (n - 1)
 *     e0 = lo + (8 b) * h,   e1 = lo + min(8 b + 8, n - 1) * h            the extent of the brick's cells
 *     g0 = e0 - margin_voxels * h,   g1 = e1 + margin_voxels * h           grown
 *   k is the smallest cascade with -s_k <= g0 and g1 <= s_k on all three axes, s_k = min(2^(k - 1), scale); the last cascade if
 *   there is none.  Per axis the cell range is c(g0) .. c(g1), c(u) = min(max(floor((u / s_k + 1) * 0.5 * G), 0), G - 1).  The brick
 *   is meshed iff a cell (cx, cy, cz) of those ranges has its bit set: bit k * G^3 + morton(cx, cy, cz) of density_bitfield, in
 *   byte >> 3 at position & 7 -- the bit the ray marcher reads.  G is a power of two, 2..1024; 1 <= cascades <= 32.
 */
#ifndef NGP_MESHSPARSE_H
#define NGP_MESHSPARSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef NGP_EINVAL
#define NGP_EINVAL   (-1)  /* bad argument (null pointer, size out of range) */
#endif
#ifndef NGP_ERANGE
#define NGP_ERANGE   (-5)  /* the mesh has more than INT32_MAX vertices or faces: its indices do not fit int32 */
#endif

#define NGP_MESHSPARSE_BRICK 8          /* lattice points per brick and axis */
#define NGP_MESHSPARSE_BRICK_POINTS 512 /* pool entries per sample slot */

/* ABI version of this library (1). */
int ngp_meshsparse_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshsparse_build_arch(void);

/* Mesh mask (one byte per brick, 1 or 0) from the occupancy bitfield, by the rule above.  margin_voxels is finite and >= 0. */
int ngp_meshsparse_mask(const uint8_t* density_bitfield, int cascades, int grid_size, float scale, int nx, int ny, int nz,
                        const float* bounds6, double margin_voxels, uint8_t* mesh_mask, void* stream);

/* Device workspace of ngp_meshsparse_index_count / _fill: with B bricks and K = ceil(B / 2048) blocks, align256(B) + align256(4 K) +
 * 2 align256(8 K) bytes (the sample mask, and per block the packed counts and the two offsets).  0 if a size is out of range. */
size_t ngp_meshsparse_index_workspace_bytes(int nx, int ny, int nz);

/* Dilates mesh_mask to the sample mask and counts both.  counts: DEVICE int64[2] = {meshed bricks, sampled bricks}; the caller
 * reads it once to size the lists of ngp_meshsparse_index_fill. */
int ngp_meshsparse_index_count(const uint8_t* mesh_mask, int nx, int ny, int nz, void* workspace, size_t workspace_bytes,
                               int64_t* counts, void* stream);

/* After ngp_meshsparse_index_count on the same mask and workspace: brick_table (one int32 per brick), mesh_bricks (n_mesh) and
 * sample_bricks (n_sample), the counts of that call and the capacity of the lists: nothing is written past them. */
int ngp_meshsparse_index_fill(const uint8_t* mesh_mask, int nx, int ny, int nz, void* workspace, size_t workspace_bytes,
                              int64_t n_mesh, int64_t n_sample, int32_t* brick_table, int32_t* mesh_bricks, int32_t* sample_bricks,
                              void* stream);

/* World coordinates of the points of the sample slots begin .. begin+count-1: xyz (count * 512, 3) f32, the expression of
 * ngp_mesh_lattice_points.  A point of a partial brick past the lattice's end repeats the last valid coordinate of its axis. */
int ngp_meshsparse_points(int nx, int ny, int nz, const float* bounds6, const int32_t* sample_bricks, int64_t n_sample, int64_t begin,
                          int64_t count, float* xyz, void* stream);

/* Device workspace of ngp_meshsparse_count / _emit for n_mesh meshed and n_sample sampled bricks (1 <= n_sample <= 2^30,
 * 0 <= n_mesh <= n_sample): align256(512 n_sample) + align256(2048 n_sample) + align256(4 n_sample) + 2 align256(8 n_sample)
 * bytes -- per sampled point a flag byte and an int32 vertex offset, per sampled brick the packed counts and two int64 offsets.
 * 0 if a count is out of range. */
size_t ngp_meshsparse_workspace_bytes(int64_t n_mesh, int64_t n_sample);

/* Pass 1: per sampled point which of its +x, +y, +z edges carry a vertex of the result, per meshed cell its triangles, and the
 * scan of the per-brick counts.  mesh_mask is the mask brick_table and the lists were made from.
 * totals: DEVICE int64[2] = {vertices, faces}; the caller reads it once to size the outputs of ngp_meshsparse_emit. */
int ngp_meshsparse_count(const float* pool, int nx, int ny, int nz, float threshold, const uint8_t* mesh_mask, const int32_t* brick_table,
                         const int32_t* mesh_bricks, int64_t n_mesh, const int32_t* sample_bricks, int64_t n_sample, void* workspace,
                         size_t workspace_bytes, int64_t* totals, void* stream);

/* Pass 2 (after ngp_meshsparse_count with the same arguments and workspace): vertices (n_vertices, 3) f32, normals
 * (n_vertices, 3) f32 (may be NULL), vertex_key (n_vertices) i64 (may be NULL), faces (n_faces, 3) i32, face_cell (n_faces) i64
 * (may be NULL), in the raw order.  n_vertices / n_faces are the totals of pass 1 and the capacity of the outputs: nothing is
 * written past them.  NGP_ERANGE if either exceeds INT32_MAX. */
int ngp_meshsparse_emit(const float* pool, int nx, int ny, int nz, float threshold, const float* bounds6, const int32_t* brick_table,
                        const int32_t* mesh_bricks, int64_t n_mesh, const int32_t* sample_bricks, int64_t n_sample, void* workspace,
                        size_t workspace_bytes, int64_t n_vertices, int64_t n_faces, float* vertices, float* normals, int64_t* vertex_key,
                        int32_t* faces, int64_t* face_cell, void* stream);

#ifdef __cplusplus
}
#endif

#endif
