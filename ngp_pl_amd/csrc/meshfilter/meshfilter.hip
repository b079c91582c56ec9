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
// Filtering, blocks of BLOCK_ITEMS consecutive faces / vertices so that a block's output is one contiguous range:
//   mf_mark_faces    kept faces per block; marks the vertices a kept face references;
//   mf_count_vertices  marked vertices per block;
//   mf_scan_blocks   one workgroup: exclusive int64 scans of both count arrays, totals to the caller;
//   mf_emit_vertices scans the marks within the block, writes each kept vertex's attributes and its new index;
//   mf_emit_faces    scans the kept faces within the block, writes them through the new indices.
// Workspace: 5 B per vertex + 12 B per block.  Integer atomics and index order only: every output is bit-identical run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/ngp_meshfilter.h"

#define NGP_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int THREADS = 256;
constexpr int ITERS = 8;
constexpr int BLOCK_ITEMS = THREADS * ITERS;
constexpr int SCAN_THREADS = 1024;

__device__ inline int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// reads face f; false if an index is outside [0, n_v)
__device__ inline bool load_face(const int* __restrict__ faces, long long f, unsigned n_v, int v[3]) {
    v[0] = faces[3 * f];
    v[1] = faces[3 * f + 1];
    v[2] = faces[3 * f + 2];
    return (unsigned)v[0] < n_v && (unsigned)v[1] < n_v && (unsigned)v[2] < n_v;
}

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
    // wave-uniform loop over the distinct labels present: one atomic per label and wave
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(l >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int cur = __shfl(l, leader, 64);
        const unsigned long long same = __ballot(l == cur);
        if (lane == leader && atomicAdd(component_faces + cur, __popcll(same)) == 0) atomicAdd(n_components, 1ull);
        todo &= ~same;
    }
}

// block sum over THREADS threads
__device__ inline int block_sum(int acc, int* lds4) {
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = acc;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int q = 0; q < THREADS / 64; ++q) total += lds4[q];
    return total;
}

// exclusive prefix of v over the THREADS threads of the block, and the block total
__device__ inline int block_exscan(int v, int& total, int* lds4) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds4[w] = x;
    __syncthreads();
    int pre = 0;
    total = 0;
#pragma unroll
    for (int q = 0; q < THREADS / 64; ++q) {
        int s = lds4[q];
        pre += q < w ? s : 0;
        total += s;
    }
    __syncthreads();
    return pre + x - v;
}

// face f is kept iff its indices are in range and the label of its first vertex is kept
__device__ inline bool face_kept(const int* __restrict__ faces, const int* __restrict__ label, const uint8_t* __restrict__ keep,
                                 long long f, long long n_v, long long n_f, int v[3]) {
    if (f >= n_f || !load_face(faces, f, (unsigned)n_v, v)) return false;
    const int l = label[v[0]];
    return (unsigned)l < (unsigned)n_v && keep[l] != 0;
}

__global__ __launch_bounds__(THREADS) void mf_mark_faces(const int* __restrict__ faces, const int* __restrict__ label,
                                                         const uint8_t* __restrict__ keep, long long n_v, long long n_f,
                                                         uint8_t* __restrict__ used, int* __restrict__ face_counts) {
    __shared__ int lds4[THREADS / 64];
    const long long base = (long long)blockIdx.x * BLOCK_ITEMS;
    int acc = 0;
    for (int r = 0; r < ITERS; ++r) {
        const long long f = base + r * THREADS + threadIdx.x;
        int v[3];
        if (!face_kept(faces, label, keep, f, n_v, n_f, v)) continue;
        used[v[0]] = 1;                                 // every writer stores the same byte
        used[v[1]] = 1;
        used[v[2]] = 1;
        ++acc;
    }
    const int total = block_sum(acc, lds4);
    if (threadIdx.x == 0) face_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(THREADS) void mf_count_vertices(const uint8_t* __restrict__ used, long long n_v, int* __restrict__ vertex_counts) {
    __shared__ int lds4[THREADS / 64];
    const long long base = (long long)blockIdx.x * BLOCK_ITEMS;
    int acc = 0;
    for (int r = 0; r < ITERS; ++r) {
        const long long v = base + r * THREADS + threadIdx.x;
        if (v < n_v) acc += used[v] != 0;
    }
    const int total = block_sum(acc, lds4);
    if (threadIdx.x == 0) vertex_counts[blockIdx.x] = total;
}

// exclusive int64 scan of counts[0..nb) into offsets by the whole workgroup; returns the total
__device__ inline long long scan_array(const int* __restrict__ counts, int nb, long long* __restrict__ offsets, long long (*s)[SCAN_THREADS]) {
    const int t = threadIdx.x;
    const int per = (nb + SCAN_THREADS - 1) / SCAN_THREADS;
    const int b0 = min(nb, t * per), b1 = min(nb, b0 + per);
    long long mine = 0;
    for (int b = b0; b < b1; ++b) mine += counts[b];
    int cur = 0;
    s[0][t] = mine;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {        // inclusive Hillis-Steele over the per-thread sums
        long long a = s[cur][t];
        if (t >= o) a += s[cur][t - o];
        s[cur ^ 1][t] = a;
        cur ^= 1;
        __syncthreads();
    }
    long long off = s[cur][t] - mine;
    for (int b = b0; b < b1; ++b) {
        offsets[b] = off;
        off += counts[b];
    }
    const long long total = s[cur][SCAN_THREADS - 1];
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(SCAN_THREADS) void mf_scan_blocks(const int* __restrict__ vertex_counts, int nbv, long long* __restrict__ vertex_offsets,
                                                               const int* __restrict__ face_counts, int nbf, long long* __restrict__ face_offsets,
                                                               long long* __restrict__ totals) {
    __shared__ long long s[2][SCAN_THREADS];
    const long long tv = scan_array(vertex_counts, nbv, vertex_offsets, s);
    const long long tf = scan_array(face_counts, nbf, face_offsets, s);
    if (threadIdx.x == 0) {
        totals[0] = tv;
        totals[1] = tf;
    }
}

__device__ inline void copy3(const float* __restrict__ src, float* __restrict__ dst, long long from, long long to) {
    const uint32_t* s = (const uint32_t*)src + 3 * from;
    uint32_t* d = (uint32_t*)dst + 3 * to;
    d[0] = s[0];
    d[1] = s[1];
    d[2] = s[2];
}

__global__ __launch_bounds__(THREADS) void mf_emit_vertices(const uint8_t* __restrict__ used, const long long* __restrict__ vertex_offsets,
                                                            long long n_v, long long cap, const float* __restrict__ vertices,
                                                            const float* __restrict__ normals, const float* __restrict__ colors,
                                                            int* __restrict__ remap, float* __restrict__ vertices_out,
                                                            float* __restrict__ normals_out, float* __restrict__ colors_out) {
    __shared__ int lds4[THREADS / 64];
    const long long base = (long long)blockIdx.x * BLOCK_ITEMS;
    long long carry = vertex_offsets[blockIdx.x];
    for (int r = 0; r < ITERS; ++r) {
        const long long v = base + r * THREADS + threadIdx.x;
        const int k = v < n_v && used[v] != 0;         // block-uniform loop: every thread takes part in the scan
        int total;
        const long long nv = carry + block_exscan(k, total, lds4);
        carry += total;
        if (!k || nv >= cap) continue;
        remap[v] = (int)nv;                             // fits: the caller's total is <= n_vertices <= INT32_MAX
        copy3(vertices, vertices_out, v, nv);
        if (normals && normals_out) copy3(normals, normals_out, v, nv);
        if (colors && colors_out) copy3(colors, colors_out, v, nv);
    }
}

__global__ __launch_bounds__(THREADS) void mf_emit_faces(const int* __restrict__ faces, const int* __restrict__ label,
                                                         const uint8_t* __restrict__ keep, long long n_v, long long n_f,
                                                         const long long* __restrict__ face_offsets, const int* __restrict__ remap,
                                                         long long cap, int* __restrict__ faces_out) {
    __shared__ int lds4[THREADS / 64];
    const long long base = (long long)blockIdx.x * BLOCK_ITEMS;
    long long carry = face_offsets[blockIdx.x];
    for (int r = 0; r < ITERS; ++r) {
        const long long f = base + r * THREADS + threadIdx.x;
        int v[3];
        const int k = face_kept(faces, label, keep, f, n_v, n_f, v);
        int total;
        const long long nf = carry + block_exscan(k, total, lds4);
        carry += total;
        if (!k || nf >= cap) continue;
        faces_out[3 * nf] = remap[v[0]];
        faces_out[3 * nf + 1] = remap[v[1]];
        faces_out[3 * nf + 2] = remap[v[2]];
    }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

bool sizes_ok(int64_t n_v, int64_t n_f) { return n_v >= 0 && n_f >= 0 && n_v <= INT32_MAX && n_f <= INT32_MAX; }

inline long long blocks_of(long long n, int per) { return (n + per - 1) / per; }

struct Layout {
    size_t used, remap, vcounts, fcounts, voffsets, foffsets, total;
    long long nbv, nbf;
};

// at least one block of each kind, so that no size in range needs 0 bytes
Layout layout(long long n_v, long long n_f) {
    Layout l;
    l.nbv = n_v ? blocks_of(n_v, BLOCK_ITEMS) : 1;
    l.nbf = n_f ? blocks_of(n_f, BLOCK_ITEMS) : 1;
    l.used = 0;
    l.remap = align256((size_t)n_v);
    l.vcounts = l.remap + align256((size_t)n_v * 4);
    l.fcounts = l.vcounts + align256((size_t)l.nbv * 4);
    l.voffsets = l.fcounts + align256((size_t)l.nbf * 4);
    l.foffsets = l.voffsets + align256((size_t)l.nbv * 8);
    l.total = l.foffsets + (size_t)l.nbf * 8;
    return l;
}

int launched() { return (int)hipGetLastError(); }

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
    const long long n_v = n_vertices, n_f = n_faces;
    const Layout l = layout(n_v, n_f);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* used = (uint8_t*)(ws + l.used);
    int* vcounts = (int*)(ws + l.vcounts);
    int* fcounts = (int*)(ws + l.fcounts);
    // marks, new indices and block counts start at 0 (an empty side has one block, which no kernel counts)
    const hipError_t e = hipMemsetAsync(ws, 0, l.voffsets, s);
    if (e != hipSuccess) return (int)e;
    if (n_f && n_v) hipLaunchKernelGGL(mf_mark_faces, dim3((unsigned)l.nbf), dim3(THREADS), 0, s, faces, vertex_label, keep, n_v, n_f, used, fcounts);
    if (n_v) hipLaunchKernelGGL(mf_count_vertices, dim3((unsigned)l.nbv), dim3(THREADS), 0, s, (const uint8_t*)used, n_v, vcounts);
    hipLaunchKernelGGL(mf_scan_blocks, dim3(1), dim3(SCAN_THREADS), 0, s, (const int*)vcounts, (int)l.nbv, (long long*)(ws + l.voffsets),
                       (const int*)fcounts, (int)l.nbf, (long long*)(ws + l.foffsets), (long long*)totals);
    return launched();
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
    const long long n_v = n_vertices, n_f = n_faces;
    const Layout l = layout(n_v, n_f);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    int* remap = (int*)(ws + l.remap);
    if (out_vertices > 0)
        hipLaunchKernelGGL(mf_emit_vertices, dim3((unsigned)l.nbv), dim3(THREADS), 0, s, (const uint8_t*)(ws + l.used),
                           (const long long*)(ws + l.voffsets), n_v, (long long)out_vertices, vertices, normals, colors, remap, vertices_out,
                           normals_out, colors_out);
    if (out_faces > 0)
        hipLaunchKernelGGL(mf_emit_faces, dim3((unsigned)l.nbf), dim3(THREADS), 0, s, faces, vertex_label, keep, n_v, n_f,
                           (const long long*)(ws + l.foffsets), (const int*)remap, (long long)out_faces, faces_out);
    return launched();
}
