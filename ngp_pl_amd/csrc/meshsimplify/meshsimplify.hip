// libngp_meshsimplify.so: simplification of an indexed triangle mesh by vertex clustering on a uniform grid (C ABI and the exact
// rule: include/ngp_meshsimplify.h).  Compiled with -ffp-contract=off: every f32 and f64 expression below is the header's,
// operation by operation.
//
// ngp_meshsimplify_cluster, on the caller's stream:
//   clear            keys to -1, leaders to INT32_MAX, the cluster counter and the sums to 0;
//   cs_insert        one thread per vertex: its key into an open-addressing table (capacity = the power of two >= 2 V, linear
//                    probing, the key claimed by a 64-bit atomicCAS from -1), atomicMin of its index into the slot's leader; the
//                    slot is parked in vertex_label;
//   cs_sums          vertex_label = the slot's leader, now final; n, P, N and C of the vertex go to the leader's ten int64 sums.
//                    The vertices of a wave are grouped by label with the ballots of ../mesh_labels.h: a group of FOLD_MIN lanes
//                    or more is summed across the wave and added by one lane (a heavy cluster would otherwise serialise 64 adds
//                    per instruction on one address), a smaller group adds lane by lane.  Leaders are counted, one add per wave.
// ngp_meshsimplify_count:
//   sf_face_labels   the label triple of every face, (-1, -1, -1) for one that does not survive;
//   sf_dedupe_insert a second table whose slots hold a face INDEX (empty = INT32_MAX): a face compares its sorted triple with that
//                    of the face in the slot; equal: atomicMin of its own index, different: probe on, empty: atomicCAS its index
//                    in and look at the slot again if the CAS lost.  A slot's key never changes once set, so the slot ends at
//                    the group's smallest index whatever the interleaving;
//   sf_dedupe_resolve a face whose lookup does not return itself overwrites its triple with (-1, -1, -1);
//   then pass 1 of ../mesh_compact.h over the label triples as if they were the faces of a mesh of V vertices, every face kept
//   (load_face drops the -1 triples): the marks land on the leaders, the numbering is in label order.
// ngp_meshsimplify_emit:
//   sf_finish        position, normal and colour of every marked leader from its sums, in f64, rounded once;
//   then pass 2 of ../mesh_compact.h, which copies those attributes and re-indexes the faces.
// Integer atomics and index order only: every output is bit-identical run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/ngp_meshsimplify.h"

namespace {

#include "../mesh_compact.h"
#include "../mesh_cells.h"
#include "../mesh_labels.h"
#include "../mesh_mix.h"

constexpr int SUMS = 10;                                // per leader: n, P[3], N[3], C[3]
constexpr long long NO_KEY = -1;
constexpr int NO_FACE = INT32_MAX;

typedef unsigned long long u64;

__device__ inline long long fixed(float x, float lo) {
    if (x != x) return 0;
    return (long long)rintf(fminf(fmaxf(x, lo), 1.0f) * QF);
}

__global__ __launch_bounds__(THREADS) void cs_insert(const float* __restrict__ vertices, long long n_v, const float* __restrict__ origin,
                                                     float cell, long long* keys, int* leader, unsigned mask, int* __restrict__ slot_of) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_v) return;
    const Grid g = load_grid(origin, cell);
    int c[3];
    long long q[3];
    if (!cell_of(g, vertices + 3 * v, c, q)) {
        slot_of[v] = -1;
        return;
    }
    const long long key = (long long)c[0] | (long long)c[1] << 21 | (long long)c[2] << 42;
    unsigned s = (unsigned)mix((u64)key) & mask;
    for (;;) {                                          // ends: the table has more slots than there are vertices
        long long k = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == NO_KEY) {
            k = (long long)atomicCAS((u64*)(keys + s), (u64)NO_KEY, (u64)key);
            if (k == NO_KEY) k = key;
        }
        if (k == key) break;
        s = (s + 1) & mask;
    }
    atomicMin(leader + s, (int)v);
    slot_of[v] = (int)s;
}

__global__ __launch_bounds__(THREADS) void cs_sums(const float* __restrict__ vertices, const float* __restrict__ normals,
                                                   const float* __restrict__ colors, long long n_v, const float* __restrict__ origin,
                                                   float cell, const int* __restrict__ leader, int* __restrict__ label, u64* sums,
                                                   u64* n_clusters) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    int l = -1;
    long long val[SUMS] = {};
    if (v < n_v) {
        const int s = label[v];                         // the slot cs_insert parked here
        if (s >= 0) l = leader[s];
        label[v] = l;
    }
    if (l >= 0) {
        const Grid g = load_grid(origin, cell);
        int c[3];
        cell_of(g, vertices + 3 * v, c, val + 1);
        val[0] = 1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (normals) val[4 + k] = fixed(normals[3 * v + k], -1.0f);
            if (colors) val[7 + k] = fixed(colors[3 * v + k], 0.0f);
        }
    }
    const u64 leaders = __ballot(l >= 0 && l == (int)v);
    if ((threadIdx.x & 63) == 0 && leaders) atomicAdd(n_clusters, (u64)__popcll(leaders));
    // one loop over the labels; the sums of absent normals and colours are skipped outright (kernel-uniform)
    for_each_label(l, [&](int cur, u64 same, int first) {
        const bool mine = l == cur;
        u64* dst = sums + (size_t)SUMS * (unsigned)cur;
        add_group<4>(mine, same, first, val, dst);
        if (normals) add_group<3>(mine, same, first, val + 4, dst + 4);
        if (colors) add_group<3>(mine, same, first, val + 7, dst + 7);
    });
}

__device__ inline void sort3(int& a, int& b, int& c) {
    int t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
}

// the sorted label triple of face f; false for a face that does not survive
__device__ inline bool sorted_triple(const int* L, long long f, int& a, int& b, int& c) {
    a = L[3 * f];
    b = L[3 * f + 1];
    c = L[3 * f + 2];
    sort3(a, b, c);
    return a >= 0;
}

__device__ inline unsigned triple_slot(int a, int b, int c, unsigned mask) {
    return (unsigned)mix(mix((u64)(unsigned)a << 32 | (unsigned)b) ^ (unsigned)c) & mask;
}

__global__ __launch_bounds__(THREADS) void sf_face_labels(const int* __restrict__ faces, const int* __restrict__ label, long long n_v,
                                                          long long n_f, int* __restrict__ L) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_f) return;
    int v[3], a = -1, b = -1, c = -1;
    if (load_face(faces, f, (unsigned)n_v, v)) {
        a = label[v[0]];
        b = label[v[1]];
        c = label[v[2]];
        const unsigned n = (unsigned)n_v;
        if (!((unsigned)a < n && (unsigned)b < n && (unsigned)c < n && a != b && b != c && a != c)) a = b = c = -1;
    }
    L[3 * f] = a;
    L[3 * f + 1] = b;
    L[3 * f + 2] = c;
}

__global__ __launch_bounds__(THREADS) void sf_dedupe_insert(const int* __restrict__ L, long long n_f, int* table, unsigned mask) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    int a, b, c;
    if (f >= n_f || !sorted_triple(L, f, a, b, c)) return;
    unsigned s = triple_slot(a, b, c, mask);
    for (;;) {                                          // ends: the table has more slots than there are faces
        int g = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g == NO_FACE) {
            g = atomicCAS(table + s, NO_FACE, (int)f);
            if (g == NO_FACE) return;
        }
        int x, y, z;                                    // g: a surviving face of this launch's L, which nobody writes here
        sorted_triple(L, g, x, y, z);
        if (x == a && y == b && z == c) {
            atomicMin(table + s, (int)f);
            return;
        }
        s = (s + 1) & mask;
    }
}

__global__ __launch_bounds__(THREADS) void sf_dedupe_resolve(int* L, long long n_f, const int* __restrict__ table, unsigned mask) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    int a, b, c;
    if (f >= n_f || !sorted_triple(L, f, a, b, c)) return;
    unsigned s = triple_slot(a, b, c, mask);
    for (;;) {
        const int g = table[s];
        if (g == (int)f || g == NO_FACE) return;        // kept (an empty slot cannot precede the face's own key)
        int x, y, z;                                    // g is its group's smallest index: a kept face, never overwritten below
        sorted_triple(L, g, x, y, z);
        if (x == a && y == b && z == c) break;
        s = (s + 1) & mask;
    }
    L[3 * f] = -1;
    L[3 * f + 1] = -1;
    L[3 * f + 2] = -1;
}

__global__ __launch_bounds__(THREADS) void sf_finish(const float* __restrict__ vertices, long long n_v, const float* __restrict__ origin,
                                                     float cell, const uint8_t* __restrict__ used, const long long* __restrict__ sums,
                                                     float* __restrict__ position, float* __restrict__ normal, float* __restrict__ color) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_v || !used[v]) return;
    const Grid g = load_grid(origin, cell);
    int c[3];
    long long q[3];
    cell_of(g, vertices + 3 * v, c, q);                 // the leader is a member: its cell is the cluster's
    const long long* s = sums + (size_t)SUMS * v;
    const double n = (double)s[0];
#pragma unroll
    for (int k = 0; k < 3; ++k) position[3 * v + k] = (float)((double)g.o[k] + ((double)c[k] + ((double)s[1 + k] / n) / QD) * (double)g.cell);
    if (normal) {
        const double n0 = (double)s[4], n1 = (double)s[5], n2 = (double)s[6];
        const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
        normal[3 * v] = len == 0.0 ? 0.f : (float)(n0 / len);
        normal[3 * v + 1] = len == 0.0 ? 0.f : (float)(n1 / len);
        normal[3 * v + 2] = len == 0.0 ? 0.f : (float)(n2 / len);
    }
    if (color) {
#pragma unroll
        for (int k = 0; k < 3; ++k) color[3 * v + k] = (float)(((double)s[7 + k] / n) / QD);
    }
}

// every label triple that load_face accepts is a face of the output
struct AllKeep {
    __device__ bool operator()(const int*) const { return true; }
};

// the power of two >= 2 n, at least 64, at most 2^31 (still more slots than n <= INT32_MAX entries)
inline size_t table_slots(long long n) {
    size_t t = 64;
    while (t < 2 * (size_t)n && t < ((size_t)1 << 31)) t <<= 1;
    return t;
}

struct SLayout {
    size_t keys, leader, counter, sums, position, normal, color, vertex_part, labels, ftable, compact, total;
    size_t vslots, fslots;
};

// the part up to vertex_part depends on n_v alone
inline SLayout slayout(long long n_v, long long n_f) {
    SLayout l;
    l.vslots = table_slots(n_v);
    l.fslots = table_slots(n_f);
    l.keys = 0;
    l.leader = l.keys + l.vslots * 8;
    l.counter = l.leader + l.vslots * 4;
    l.sums = l.counter + 256;
    l.position = l.sums + align256((size_t)n_v * SUMS * 8);
    l.normal = l.position + align256((size_t)n_v * 12);
    l.color = l.normal + align256((size_t)n_v * 12);
    l.vertex_part = l.color + align256((size_t)n_v * 12);
    l.labels = l.vertex_part;
    l.ftable = l.labels + align256((size_t)n_f * 12);
    l.compact = l.ftable + l.fslots * 4;
    l.total = l.compact + layout(n_v, n_f).total;
    return l;
}

}  // namespace

NGP_API int ngp_meshsimplify_abi_version(void) { return 1; }

NGP_API const char* ngp_meshsimplify_build_arch(void) { return "gfx950"; }

NGP_API size_t ngp_meshsimplify_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    if (!sizes_ok(n_vertices, n_faces)) return 0;
    return slayout(n_vertices, n_faces).total;
}

NGP_API int ngp_meshsimplify_cluster(const float* vertices, const float* normals, const float* colors, int64_t n_vertices,
                                     const float* origin, float cell, void* workspace, size_t workspace_bytes, int32_t* vertex_label,
                                     void* stream) {
    if (n_vertices < 0 || !cell_ok(cell)) return NGP_EINVAL;
    if (n_vertices > INT32_MAX) return NGP_ERANGE;
    if (n_vertices == 0) return 0;
    if (!vertices || !origin || !workspace || !vertex_label) return NGP_EINVAL;
    const SLayout l = slayout(n_vertices, 0);
    if (workspace_bytes < l.vertex_part) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const long long n_v = n_vertices;
    hipError_t e = hipMemsetAsync(ws + l.keys, 0xFF, l.vslots * 8, s);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)(ws + l.leader), INT32_MAX, l.vslots, s);
    if (e == hipSuccess) e = hipMemsetAsync(ws + l.counter, 0, l.position - l.counter, s);
    if (e != hipSuccess) return (int)e;
    const unsigned vb = (unsigned)blocks_of(n_v, THREADS);
    hipLaunchKernelGGL(cs_insert, dim3(vb), dim3(THREADS), 0, s, vertices, n_v, origin, cell, (long long*)(ws + l.keys), (int*)(ws + l.leader),
                       (unsigned)(l.vslots - 1), vertex_label);
    hipLaunchKernelGGL(cs_sums, dim3(vb), dim3(THREADS), 0, s, vertices, normals, colors, n_v, origin, cell, (const int*)(ws + l.leader),
                       vertex_label, (u64*)(ws + l.sums), (u64*)(ws + l.counter));
    return launched();
}

NGP_API int ngp_meshsimplify_count(const int32_t* faces, const int32_t* vertex_label, int64_t n_vertices, int64_t n_faces, void* workspace,
                                   size_t workspace_bytes, int64_t* totals, void* stream) {
    if (n_vertices < 0 || n_faces < 0) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (n_vertices == 0) return 0;
    if (!workspace || !totals || !vertex_label || (n_faces > 0 && !faces)) return NGP_EINVAL;
    const SLayout l = slayout(n_vertices, n_faces);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const long long n_v = n_vertices, n_f = n_faces;
    int* L = (int*)(ws + l.labels);
    if (n_f) {
        int* table = (int*)(ws + l.ftable);
        const unsigned fb = (unsigned)blocks_of(n_f, THREADS), mask = (unsigned)(l.fslots - 1);
        const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)table, NO_FACE, l.fslots, s);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(sf_face_labels, dim3(fb), dim3(THREADS), 0, s, faces, vertex_label, n_v, n_f, L);
        hipLaunchKernelGGL(sf_dedupe_insert, dim3(fb), dim3(THREADS), 0, s, (const int*)L, n_f, table, mask);
        hipLaunchKernelGGL(sf_dedupe_resolve, dim3(fb), dim3(THREADS), 0, s, L, n_f, (const int*)table, mask);
    }
    const int rc = compact_count(AllKeep{}, (const int*)L, n_v, n_f, ws + l.compact, (long long*)totals, s);
    if (rc != 0) return rc;
    return (int)hipMemcpyAsync(totals + 2, ws + l.counter, 8, hipMemcpyDeviceToDevice, s);
}

NGP_API int ngp_meshsimplify_emit(const float* vertices, int64_t n_vertices, int64_t n_faces, const float* origin, float cell,
                                  void* workspace, size_t workspace_bytes, int64_t out_vertices, int64_t out_faces, float* vertices_out,
                                  float* normals_out, float* colors_out, int32_t* faces_out, void* stream) {
    if (n_vertices < 0 || n_faces < 0 || out_vertices < 0 || out_faces < 0 || !cell_ok(cell)) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (out_vertices > n_vertices || out_faces > n_faces) return NGP_EINVAL;
    if (out_vertices == 0 && out_faces == 0) return 0;
    if (!workspace || !vertices || !origin) return NGP_EINVAL;
    if (out_vertices > 0 && !vertices_out) return NGP_EINVAL;
    if (out_faces > 0 && !faces_out) return NGP_EINVAL;
    const SLayout l = slayout(n_vertices, n_faces);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const long long n_v = n_vertices;
    float* position = (float*)(ws + l.position);
    float* normal = normals_out ? (float*)(ws + l.normal) : nullptr;
    float* color = colors_out ? (float*)(ws + l.color) : nullptr;
    if (out_vertices > 0)
        hipLaunchKernelGGL(sf_finish, dim3((unsigned)blocks_of(n_v, THREADS)), dim3(THREADS), 0, s, vertices, n_v, origin, cell,
                           (const uint8_t*)(ws + l.compact + layout(n_v, n_faces).used), (const long long*)(ws + l.sums), position, normal, color);
    return compact_emit(AllKeep{}, (const int*)(ws + l.labels), (const float*)position, (const float*)normal, (const float*)color, n_v, n_faces,
                        ws + l.compact, out_vertices, out_faces, vertices_out, normals_out, colors_out, faces_out, s);
}
