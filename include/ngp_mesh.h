/*
 * ngp_mesh.h -- C ABI of libngp_mesh.so: surface extraction (marching cubes) over a sampled density volume, on gfx950.
 *
 * Mesh export is not part of the drop-in boundary of include/ngp_hip.h, so it lives in a library of its own with the same
 * conventions: raw DEVICE pointers, caller-allocated outputs and workspace, the hipStream_t passed as void*, 0 on success, a
 * positive hipError_t if a launch failed, a negative NGP_E* code for bad arguments.  No entry point allocates or synchronises.
 *
 * Volume layout: f32 (nz, ny, nx), x fastest; lattice point (i, j, k) has linear index (k*ny + j)*nx + i and sits at
 * lo + (i, j, k) * (hi - lo) / (n - 1) per axis.  bounds6 is a HOST pointer to {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z}.
 * Cell (i, j, k) spans points i..i+1, j..j+1, k..k+1.  A point is inside iff sigma > threshold.
 *
 * Output (deterministic, bit-identical run to run and for any launch configuration):
 *   - one vertex per edge with exactly one inside endpoint; a lattice point owns its +x, +y, +z edges and vertices are numbered
 *     by (owning point's linear index, axis x < y < z).  With a = the owning endpoint, t = clamp((thr - sa) / (sb - sa), 0, 1)
 *     and the vertex is pa + t * (pb - pa);
 *   - normals: the central-difference gradient of the volume (one-sided at the border, per-axis spacing) at both endpoints,
 *     interpolated with t; n = -g / |g| (outward), 0 for a zero gradient;
 *   - faces (F, 3) i32, indexed into the vertices, numbered by (cell linear index, table order of ngp_pl_amd/csrc/mesh/mc_tables.h),
 *     counter-clockwise seen from outside.
 */
#ifndef NGP_MESH_H
#define NGP_MESH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef NGP_EINVAL
#define NGP_EINVAL   (-1)  /* bad argument (null pointer, size out of range) */
#endif
#define NGP_ERANGE   (-5)  /* the mesh has more than INT32_MAX vertices or faces: its indices do not fit int32 */

/* ABI version of this library (1). */
int ngp_mesh_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_mesh_build_arch(void);

/* Device workspace ngp_mesh_count / ngp_mesh_emit need for an nx x ny x nz volume: 5 bytes per lattice point (a flag byte and
 * an int32 vertex offset) plus 20 bytes per brick of 2048 points.  0 if a size is out of range (each axis 2..65535, at most
 * 2^36 points). */
size_t ngp_mesh_workspace_bytes(int nx, int ny, int nz);

/* World coordinates of the lattice points begin .. begin+count-1 (linear order): xyz (count, 3) f32. */
int ngp_mesh_lattice_points(int nx, int ny, int nz, const float* bounds6, int64_t begin, int64_t count, float* xyz, void* stream);

/* Pass 1: classifies every point and cell, counts per brick and scans the brick counts on the device.
 * totals: DEVICE int64[2] = {vertices, faces}; the caller reads it once to size the outputs of ngp_mesh_emit. */
int ngp_mesh_count(const float* volume, int nx, int ny, int nz, float threshold, void* workspace, size_t workspace_bytes,
                   int64_t* totals, void* stream);

/* Pass 2 (after ngp_mesh_count on the same volume, threshold and workspace): writes vertices (n_vertices, 3) f32, normals
 * (n_vertices, 3) f32 (may be NULL) and faces (n_faces, 3) i32.  n_vertices / n_faces are the totals of ngp_mesh_count and the
 * capacity of the outputs: nothing is written past them.  NGP_ERANGE if either exceeds INT32_MAX. */
int ngp_mesh_emit(const float* volume, int nx, int ny, int nz, float threshold, const float* bounds6, void* workspace,
                  size_t workspace_bytes, int64_t n_vertices, int64_t n_faces, float* vertices, float* normals, int32_t* faces,
                  void* stream);

#ifdef __cplusplus
}
#endif

#endif
