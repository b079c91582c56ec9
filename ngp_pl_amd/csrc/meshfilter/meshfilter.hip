// libngp_meshfilter.so: connected components of an indexed triangle mesh and the sub-mesh of kept components
// (C ABI: include/ngp_meshfilter.h).
//
// Labelling, four launches on the caller's stream, the parent array being the caller's vertex_label:
//   uf_init          parent[v] = v, component_faces[v] = 0, the component counter = 0;
//   uf_union         one face per thread unions (v0, v1) and (v0, v2): roots by path halving, the larger root hooked under the
//                    smaller with atomicCAS, again from where the CAS lost.  parent[x] <= x always and a root only ever gains a
//                    smaller parent, so one pass over the faces is complete and the surviving root is the component's minimum;
//   uf_flatten       parent[v] = root(v);
//   uf_face_labels   face_label = label of the first vertex; the faces of a wave are grouped by label with ballots and one
//                    lane per distinct label adds the group's size (marching cubes numbers faces by cell: a wave nearly always
//                    holds one label).  The add that finds 0 counts the component.
// Filtering is the shared compaction of ../mesh_compact.h (mf_mark_faces, mf_count_vertices, mf_scan_blocks, mf_emit_vertices,
// mf_emit_faces) with the rule LabelKeep: a face is kept iff the label of its first vertex is kept.
// Workspace: 5 B per vertex + 12 B per block.  Integer atomics and index order only: every output is bit-identical run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/ngp_meshfilter.h"

namespace {

#include "../mesh_compact.h"
#include "../mesh_labels.h"

__device__ inline int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x by path halving; parent[x] only ever moves to a smaller ancestor (atomicMin), whichever thread gets there first
__device__ inline int find_root(int* parent, int x) {
    for (;;) {
        const int p = ld(parent + x);
        if (p == x) return x;
        const int g = ld(parent + p);
        if (g == p) return p;
        atomicMin(parent + x, g);
        x = g;
    }
}

__device__ inline void unite(int* parent, int a, int b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;                                        // hi was hooked elsewhere meanwhile: go on from its new parent
        b = lo;
    }
}

__global__ __launch_bounds__(THREADS) void uf_init(long long n_v, int* __restrict__ parent, int* __restrict__ component_faces,
                                                   unsigned long long* __restrict__ n_components) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (v == 0) *n_components = 0;
    if (v >= n_v) return;
    parent[v] = (int)v;
    component_faces[v] = 0;
}

__global__ __launch_bounds__(THREADS) void uf_union(const int* __restrict__ faces, long long n_v, long long n_f, int* parent) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    int v[3];
    if (f >= n_f || !load_face(faces, f, (unsigned)n_v, v)) return;
    unite(parent, v[0], v[1]);
    unite(parent, v[0], v[2]);
}

__global__ __launch_bounds__(THREADS) void uf_flatten(long long n_v, int* parent) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_v) return;
    const int r = find_root(parent, (int)v);
    if (r != (int)v) atomicMin(parent + v, r);
}

__global__ __launch_bounds__(THREADS) void uf_face_labels(const int* __restrict__ faces, const int* __restrict__ label, long long n_v,
                                                          long long n_f, int* __restrict__ face_label, int* component_faces,
                                                          unsigned long long* n_components) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    int l = -1;
    if (f < n_f) {
        int v[3];
        if (load_face(faces, f, (unsigned)n_v, v)) l = label[v[0]];
        face_label[f] = l;
    }
    // one atomic per distinct label and wave
    for_each_label(l, [&](int cur, unsigned long long same, int first) {
        if ((int)(threadIdx.x & 63) == first && atomicAdd(component_faces + cur, __popcll(same)) == 0) atomicAdd(n_components, 1ull);
    });
}

// the filter's rule: the label of the face's first vertex is kept
struct LabelKeep {
    const int* label;
    const uint8_t* keep;
    unsigned n_v;
    __device__ bool operator()(const int v[3]) const {
        const int l = label[v[0]];
        return (unsigned)l < n_v && keep[l] != 0;
    }
};

}  // namespace

NGP_API int ngp_meshfilter_abi_version(void) { return 1; }

NGP_API const char* ngp_meshfilter_build_arch(void) { return "gfx950"; }

NGP_API size_t ngp_meshfilter_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    if (!sizes_ok(n_vertices, n_faces)) return 0;
    return layout(n_vertices, n_faces).total;
}

NGP_API int ngp_meshfilter_label(const int32_t* faces, int64_t n_vertices, int64_t n_faces, int32_t* vertex_label, int32_t* face_label,
                                 int32_t* component_faces, int64_t* n_components, void* stream) {
    if (n_vertices < 0 || n_faces < 0) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (n_vertices == 0 && n_faces == 0) return 0;
    if (!n_components || (n_vertices > 0 && (!vertex_label || !component_faces)) || (n_faces > 0 && (!faces || !face_label))) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long n_v = n_vertices, n_f = n_faces;
    const unsigned vb = (unsigned)blocks_of(n_v, THREADS), fb = (unsigned)blocks_of(n_f, THREADS);
    unsigned long long* count = (unsigned long long*)n_components;
    hipLaunchKernelGGL(uf_init, dim3(vb ? vb : 1), dim3(THREADS), 0, s, n_v, vertex_label, component_faces, count);
    if (fb && vb) hipLaunchKernelGGL(uf_union, dim3(fb), dim3(THREADS), 0, s, faces, n_v, n_f, vertex_label);
    if (vb) hipLaunchKernelGGL(uf_flatten, dim3(vb), dim3(THREADS), 0, s, n_v, vertex_label);
    if (fb) hipLaunchKernelGGL(uf_face_labels, dim3(fb), dim3(THREADS), 0, s, faces, (const int*)vertex_label, n_v, n_f, face_label,
                               component_faces, count);
    return launched();
}

NGP_API int ngp_meshfilter_count(const int32_t* faces, const int32_t* vertex_label, const uint8_t* keep, int64_t n_vertices,
                                 int64_t n_faces, void* workspace, size_t workspace_bytes, int64_t* totals, void* stream) {
    if (n_vertices < 0 || n_faces < 0) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (n_vertices == 0 && n_faces == 0) return 0;
    if (!workspace || !totals || (n_vertices > 0 && (!vertex_label || !keep)) || (n_faces > 0 && !faces)) return NGP_EINVAL;
    if (workspace_bytes < layout(n_vertices, n_faces).total) return NGP_EINVAL;
    return compact_count(LabelKeep{vertex_label, keep, (unsigned)n_vertices}, faces, n_vertices, n_faces, (char*)workspace, (long long*)totals,
                         (hipStream_t)stream);
}

NGP_API int ngp_meshfilter_emit(const int32_t* faces, const int32_t* vertex_label, const uint8_t* keep, const float* vertices,
                                const float* normals, const float* colors, int64_t n_vertices, int64_t n_faces, void* workspace,
                                size_t workspace_bytes, int64_t out_vertices, int64_t out_faces, float* vertices_out, float* normals_out,
                                float* colors_out, int32_t* faces_out, void* stream) {
    if (n_vertices < 0 || n_faces < 0 || out_vertices < 0 || out_faces < 0) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (out_vertices > n_vertices || out_faces > n_faces) return NGP_EINVAL;
    if (out_vertices == 0 && out_faces == 0) return 0;
    if (!workspace || !vertex_label || !keep || !faces) return NGP_EINVAL;
    if (out_vertices > 0 && (!vertices || !vertices_out || !normals != !normals_out || !colors != !colors_out)) return NGP_EINVAL;
    if (out_faces > 0 && !faces_out) return NGP_EINVAL;
    if (workspace_bytes < layout(n_vertices, n_faces).total) return NGP_EINVAL;
    return compact_emit(LabelKeep{vertex_label, keep, (unsigned)n_vertices}, faces, vertices, normals, colors, n_vertices, n_faces, (char*)workspace,
                        out_vertices, out_faces, vertices_out, normals_out, colors_out, faces_out, (hipStream_t)stream);
}
