// Order-preserving compaction of an indexed triangle mesh, shared by libngp_meshfilter.so, libngp_meshcull.so,
// libngp_meshsimplify.so and libngp_meshdecimate.so: each includes this header inside its own anonymous namespace (the sums and
// scans of mesh_scan.h and the host helpers of mesh_host.h come with it) and supplies the rule that keeps a face as a functor
//     struct Keep { __device__ bool operator()(const int v[3]) const; };      // v: the face's indices, all inside [0, n_v)
// A face with an index outside [0, n_v) is never kept and nothing is read through it.  A vertex is kept when a kept face references it.
// Blocks of BLOCK_ITEMS consecutive faces / vertices, so that a block's output is one contiguous range:
//   mf_mark_faces    kept faces per block; marks the vertices a kept face references;
//   mf_count_vertices  marked vertices per block;
//   mf_scan_blocks   one workgroup: exclusive int64 scans of both count arrays, totals to the caller;
//   mf_emit_vertices scans the marks within the block, writes each kept vertex's attributes and its new index;
//   mf_emit_faces    scans the kept faces within the block, writes them through the new indices.
// Workspace: 5 B per vertex + 12 B per block.  Index order only: every output is bit-identical run to run.
#ifndef NGP_MESH_COMPACT_H
#define NGP_MESH_COMPACT_H

#include "mesh_host.h"
#include "mesh_scan.h"

constexpr int THREADS = 256;
constexpr int ITERS = 8;
constexpr int BLOCK_ITEMS = THREADS * ITERS;

// reads face f; false if an index is outside [0, n_v)
__device__ inline bool load_face(const int* __restrict__ faces, long long f, unsigned n_v, int v[3]) {
    v[0] = faces[3 * f];
    v[1] = faces[3 * f + 1];
    v[2] = faces[3 * f + 2];
    return (unsigned)v[0] < n_v && (unsigned)v[1] < n_v && (unsigned)v[2] < n_v;
}

template <class Keep>
__device__ inline bool face_kept(const Keep& keep, const int* __restrict__ faces, long long f, long long n_v, long long n_f, int v[3]) {
    return f < n_f && load_face(faces, f, (unsigned)n_v, v) && keep(v);
}

template <class Keep>
__global__ __launch_bounds__(THREADS) void mf_mark_faces(Keep keep, const int* __restrict__ faces, long long n_v, long long n_f,
                                                         uint8_t* __restrict__ used, int* __restrict__ face_counts) {
    __shared__ int lds4[THREADS / 64];
    const long long base = (long long)blockIdx.x * BLOCK_ITEMS;
    int acc = 0;
    for (int r = 0; r < ITERS; ++r) {
        const long long f = base + r * THREADS + threadIdx.x;
        int v[3];
        if (!face_kept(keep, faces, f, n_v, n_f, v)) continue;
        used[v[0]] = 1;                                 // every writer stores the same byte
        used[v[1]] = 1;
        used[v[2]] = 1;
        ++acc;
    }
    const int total = block_sum<THREADS>(acc, lds4);
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
    const int total = block_sum<THREADS>(acc, lds4);
    if (threadIdx.x == 0) vertex_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(SCAN_THREADS) void mf_scan_blocks(const int* __restrict__ vertex_counts, int nbv, long long* __restrict__ vertex_offsets,
                                                               const int* __restrict__ face_counts, int nbf, long long* __restrict__ face_offsets,
                                                               long long* __restrict__ totals) {
    __shared__ long long s[2][SCAN_THREADS];
    const long long tv = scan_array([=](long long b) { return (long long)vertex_counts[b]; }, nbv, vertex_offsets, s);
    const long long tf = scan_array([=](long long b) { return (long long)face_counts[b]; }, nbf, face_offsets, s);
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
        const long long nv = carry + block_exscan<THREADS>(k, total, lds4);
        carry += total;
        if (!k || nv >= cap) continue;
        remap[v] = (int)nv;                             // fits: the caller's total is <= n_vertices <= INT32_MAX
        copy3(vertices, vertices_out, v, nv);
        if (normals && normals_out) copy3(normals, normals_out, v, nv);
        if (colors && colors_out) copy3(colors, colors_out, v, nv);
    }
}

template <class Keep>
__global__ __launch_bounds__(THREADS) void mf_emit_faces(Keep keep, const int* __restrict__ faces, long long n_v, long long n_f,
                                                         const long long* __restrict__ face_offsets, const int* __restrict__ remap,
                                                         long long cap, int* __restrict__ faces_out) {
    __shared__ int lds4[THREADS / 64];
    const long long base = (long long)blockIdx.x * BLOCK_ITEMS;
    long long carry = face_offsets[blockIdx.x];
    for (int r = 0; r < ITERS; ++r) {
        const long long f = base + r * THREADS + threadIdx.x;
        int v[3];
        const int k = face_kept(keep, faces, f, n_v, n_f, v);
        int total;
        const long long nf = carry + block_exscan<THREADS>(k, total, lds4);
        carry += total;
        if (!k || nf >= cap) continue;
        faces_out[3 * nf] = remap[v[0]];
        faces_out[3 * nf + 1] = remap[v[1]];
        faces_out[3 * nf + 2] = remap[v[2]];
    }
}

struct Layout {
    size_t used, remap, vcounts, fcounts, voffsets, foffsets, total;
    long long nbv, nbf;
};

// at least one block of each kind, so that no size in range needs 0 bytes
inline Layout layout(long long n_v, long long n_f) {
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

// Pass 1 on stream s: marks, block counts, the device scan; totals = {kept vertices, kept faces}.  The caller has checked the
// arguments: sizes in range and not both 0, workspace of layout(n_v, n_f).total bytes.
template <class Keep>
int compact_count(const Keep& keep, const int* faces, long long n_v, long long n_f, char* ws, long long* totals, hipStream_t s) {
    const Layout l = layout(n_v, n_f);
    uint8_t* used = (uint8_t*)(ws + l.used);
    int* vcounts = (int*)(ws + l.vcounts);
    int* fcounts = (int*)(ws + l.fcounts);
    // marks, new indices and block counts start at 0 (an empty side has one block, which no kernel counts)
    const hipError_t e = hipMemsetAsync(ws, 0, l.voffsets, s);
    if (e != hipSuccess) return (int)e;
    if (n_f && n_v) hipLaunchKernelGGL(mf_mark_faces<Keep>, dim3((unsigned)l.nbf), dim3(THREADS), 0, s, keep, faces, n_v, n_f, used, fcounts);
    if (n_v) hipLaunchKernelGGL(mf_count_vertices, dim3((unsigned)l.nbv), dim3(THREADS), 0, s, (const uint8_t*)used, n_v, vcounts);
    hipLaunchKernelGGL(mf_scan_blocks, dim3(1), dim3(SCAN_THREADS), 0, s, (const int*)vcounts, (int)l.nbv, (long long*)(ws + l.voffsets),
                       (const int*)fcounts, (int)l.nbf, (long long*)(ws + l.foffsets), totals);
    return launched();
}

// Pass 2, after compact_count with the same mesh, rule and workspace; out_v / out_f are its totals and the outputs' capacity.
template <class Keep>
int compact_emit(const Keep& keep, const int* faces, const float* vertices, const float* normals, const float* colors, long long n_v,
                 long long n_f, char* ws, long long out_v, long long out_f, float* vertices_out, float* normals_out, float* colors_out,
                 int* faces_out, hipStream_t s) {
    const Layout l = layout(n_v, n_f);
    int* remap = (int*)(ws + l.remap);
    if (out_v > 0)
        hipLaunchKernelGGL(mf_emit_vertices, dim3((unsigned)l.nbv), dim3(THREADS), 0, s, (const uint8_t*)(ws + l.used),
                           (const long long*)(ws + l.voffsets), n_v, out_v, vertices, normals, colors, remap, vertices_out, normals_out,
                           colors_out);
    if (out_f > 0)
        hipLaunchKernelGGL(mf_emit_faces<Keep>, dim3((unsigned)l.nbf), dim3(THREADS), 0, s, keep, faces, n_v, n_f,
                           (const long long*)(ws + l.foffsets), (const int*)remap, out_f, faces_out);
    return launched();
}

#endif
