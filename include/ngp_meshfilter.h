/*
 * ngp_meshfilter.h -- C ABI of libngp_meshfilter.so: connected components of an indexed triangle mesh and the sub-mesh of the
 * components a caller keeps, on gfx950.
 *
 * A library of its own beside libngp_hip.so (include/ngp_hip.h) and libngp_mesh.so (include/ngp_mesh.h), with their
 * conventions: raw DEVICE pointers, caller-allocated outputs and workspace, the hipStream_t passed as void*, 0 on success, a
 * positive hipError_t if a launch failed, a negative NGP_E* code for bad arguments.  No entry point allocates or synchronises,
 * and every argument is checked on the host before anything is launched.  This header needs neither of the other two and may
 * be included after them.
 *
 * Mesh: faces (n_faces, 3) i32 index n_vertices vertices.  Two vertices are connected when some face holds both; a component is
 * a connected set of vertices with the faces on them; its label is its SMALLEST VERTEX INDEX.  A vertex that no face references
 * is a component of its own with 0 faces.  A face with an index outside [0, n_vertices) connects nothing, gets label -1, is
 * counted nowhere and is never kept; nothing is read or written through such an index.
 *
 * Every output is fixed by the mesh alone (labels are minima, counts are integer sums, the filter keeps the input's order):
 * bit-identical run to run and for any launch configuration.
 */
#ifndef NGP_MESHFILTER_H
#define NGP_MESHFILTER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef NGP_EINVAL
#define NGP_EINVAL   (-1)  /* bad argument (null pointer, negative size, workspace too small) */
#endif
#ifndef NGP_ERANGE
#define NGP_ERANGE   (-5)  /* more than INT32_MAX vertices or faces: the indices do not fit int32 */
#endif

/* ABI version of this library (1). */
int ngp_meshfilter_abi_version(void);
/* Name of the GPU arch the library was built for ("gfx950"). */
const char* ngp_meshfilter_build_arch(void);

/* Device workspace ngp_meshfilter_count / ngp_meshfilter_emit need: 5 bytes per vertex (a referenced-by-a-kept-face byte and the
 * int32 new index) plus 12 bytes per block of 2048 vertices and per block of 2048 faces (an int32 count and an int64 offset).
 * 0 if a size is out of range (negative, or above INT32_MAX).  ngp_meshfilter_label needs no workspace. */
size_t ngp_meshfilter_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* Labels the components (lock-free union-find over the faces, then a flatten pass, then the face counts):
 *   vertex_label (n_vertices) i32      label of each vertex;
 *   face_label (n_faces) i32           label of each face's first vertex (-1 for a face with an index out of range);
 *   component_faces (n_vertices) i32   at a label's own index the number of faces of that component, 0 everywhere else;
 *   n_components DEVICE int64          number of components with at least one face.
 * With n_vertices == 0 and n_faces == 0 nothing is launched and nothing is written. */
int ngp_meshfilter_label(const int32_t* faces, int64_t n_vertices, int64_t n_faces, int32_t* vertex_label, int32_t* face_label,
                         int32_t* component_faces, int64_t* n_components, void* stream);

/* Filter pass 1.  keep (n_vertices) u8 is indexed by LABEL: non-zero keeps that component.  A face is kept iff the label of its
 * first vertex is kept; a vertex is kept iff its label is kept and a kept face references it.  Counts the kept vertices and faces
 * per block and scans the block counts on the device.  totals: DEVICE int64[2] = {kept vertices, kept faces}; the caller reads it
 * once to size the outputs of ngp_meshfilter_emit.  vertex_label is the output of ngp_meshfilter_label on the same mesh.
 * With n_vertices == 0 and n_faces == 0 nothing is launched and nothing is written. */
int ngp_meshfilter_count(const int32_t* faces, const int32_t* vertex_label, const uint8_t* keep, int64_t n_vertices, int64_t n_faces,
                         void* workspace, size_t workspace_bytes, int64_t* totals, void* stream);

/* Filter pass 2 (after ngp_meshfilter_count with the same mesh, labels, keep and workspace): the kept vertices and faces in the
 * input's relative order, the faces re-indexed.  vertices / normals / colors are (n_vertices, 3) f32, copied bit for bit into
 * vertices_out / normals_out / colors_out (out_vertices, 3); normals and colors may be NULL, together with their outputs.
 * faces_out is (out_faces, 3) i32.  out_vertices / out_faces are the totals of ngp_meshfilter_count and the capacity of the
 * outputs: nothing is written past them. */
int ngp_meshfilter_emit(const int32_t* faces, const int32_t* vertex_label, const uint8_t* keep, const float* vertices,
                        const float* normals, const float* colors, int64_t n_vertices, int64_t n_faces, void* workspace,
                        size_t workspace_bytes, int64_t out_vertices, int64_t out_faces, float* vertices_out, float* normals_out,
                        float* colors_out, int32_t* faces_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
