// libngp_meshsmooth.so: Taubin smoothing of an indexed triangle mesh on an integer grid and geometric vertex normals (C ABI and
// the exact rule: include/ngp_meshsmooth.h).  Compiled with -ffp-contract=off: every f32 and f64 expression below is the
// header's, operation by operation.
//
// ngp_meshsmooth_topology, on the caller's stream:
//   clear            edge keys to all ones, occurrences, degrees, marks and totals to 0;
//   st_inside        one thread per vertex: bit 0 of its mark when the vertex is inside the grid;
//   st_insert        one thread per face: each side of a valid face whose ends are both inside goes, keyed min << 32 | max, into an
//                    open-addressing table (capacity = the power of two >= 6 F, linear probing bounded by the capacity, the key
//                    claimed by a 64-bit atomicCAS from all ones) and adds 1 to the slot's occurrences;
//   st_degrees       one thread per slot: a claimed slot is one edge: +1 to the degree of both ends, bit 1 of both marks when it
//                    occurred once (every writer ORs the same bit), edges and boundary edges counted per block;
//   st_block_sums, st_scan_blocks, st_rows   the exclusive int64 scan of the degrees (blocks of 2048 vertices, one workgroup
//                    over the block sums, then the scan inside each block): row offsets, the caller's degree and flags, the
//                    free and boundary vertices counted per block;
//   st_fill          one thread per slot: each end into the other's row, at a position handed out by counting the workspace's
//                    copy of the degree down.  The order inside a row is arbitrary: rows only ever feed integer sums.
// ngp_meshsmooth_taubin:
//   tb_state         the grid state of every vertex into BOTH ping-pong buffers (a vertex that is not free is never written again);
//   tb_pass          2 * pairs launches, a gather without atomics: one thread per free vertex walks its row and sums the
//                    neighbours' states in int64; rows longer than LONG_ROW are left to the whole wave, lane i taking entries
//                    i, i + 64, ..., and summed across the wave (integer sums: the split changes nothing);
//   tb_output        free vertices from the state, every other vertex's input words.
// ngp_meshsmooth_normals:
//   nm_faces         one thread per face: its unit normal in 2^-20 fixed point added to its three corners' int64 sums;
//   nm_finish        one thread per vertex: the sum normalised in f64.
// Integer atomics only, and none in the passes: every output is bit-identical run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/ngp_meshsmooth.h"

namespace {

#include "../mesh_host.h"
#include "../mesh_mix.h"
#include "../mesh_scan.h"

constexpr int THREADS = 256;
constexpr int ITERS = 8;
constexpr int BLOCK_ITEMS = THREADS * ITERS;            // vertices per block of the scan
constexpr int LONG_ROW = 32;                            // rows longer than this are summed by the wave
constexpr float QF = 65536.0f;                          // the header's Q
constexpr double QD = 65536.0;
constexpr float QMAXF = 1073741824.0f;                  // 2^30
constexpr int QMAX = 1 << 30;
constexpr double NQ = 1048576.0;                        // the normals' fixed point, 2^20
constexpr int INSIDE = 1, BOUNDARY = 2, FREE = 4;

typedef unsigned long long u64;
constexpr u64 NO_KEY = ~(u64)0;

// the header's grid state: false when the vertex is outside (q is then 0)
__device__ inline bool state_of(const float* __restrict__ origin, float cell, const float* __restrict__ x, int q[3]) {
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t = (x[k] - origin[k]) / cell;
        const float r = rintf(t * QF);
        const bool ok = fabsf(t) < __uint_as_float(0x7F800000u) && fabsf(r) <= QMAXF;          // false for NaN
        inside = inside && ok;
        q[k] = ok ? (int)r : 0;
    }
    if (!inside) q[0] = q[1] = q[2] = 0;
    return inside;
}

__global__ __launch_bounds__(THREADS) void st_inside(const float* __restrict__ vertices, long long n_v, const float* __restrict__ origin,
                                                     float cell, uint8_t* __restrict__ mark) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_v) return;
    int q[3];
    mark[v] = state_of(origin, cell, vertices + 3 * v, q) ? INSIDE : 0;
}

__device__ inline void insert_edge(int a, int b, u64* keys, int* occ, u64 slots) {
    const u64 key = (u64)(unsigned)min(a, b) << 32 | (unsigned)max(a, b);
    u64 s = mix(key) & (slots - 1);
    for (u64 probe = 0; probe < slots; ++probe) {       // the table has more slots than there are sides: an empty one comes first
        u64 k = __hip_atomic_load(keys + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == NO_KEY) {
            k = atomicCAS(keys + s, NO_KEY, key);
            if (k == NO_KEY) k = key;
        }
        if (k == key) {
            atomicAdd(occ + s, 1);
            return;
        }
        s = (s + 1) & (slots - 1);
    }
}

__global__ __launch_bounds__(THREADS) void st_insert(const int* __restrict__ faces, long long n_v, long long n_f,
                                                     const uint8_t* __restrict__ mark, u64* keys, int* occ, u64 slots) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_f) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const unsigned n = (unsigned)n_v;
    if (!((unsigned)a < n && (unsigned)b < n && (unsigned)c < n && a != b && b != c && a != c)) return;
    const bool ia = mark[a] & INSIDE, ib = mark[b] & INSIDE, ic = mark[c] & INSIDE;
    if (ia && ib) insert_edge(a, b, keys, occ, slots);
    if (ib && ic) insert_edge(b, c, keys, occ, slots);
    if (ic && ia) insert_edge(c, a, keys, occ, slots);
}

// a byte of `mark` gains a bit: the 32-bit word that holds it takes the OR (the workspace is 256-byte aligned and padded)
__device__ inline void mark_or(uint8_t* mark, long long v, unsigned bit) {
    atomicOr((unsigned*)(mark + (v & ~3ll)), bit << (8 * (int)(v & 3)));
}

__global__ __launch_bounds__(THREADS) void st_degrees(const u64* __restrict__ keys, const int* __restrict__ occ, u64 slots, int* degree,
                                                      uint8_t* mark, u64* totals) {
    __shared__ long long lds4[THREADS / 64];
    const u64 s = (u64)blockIdx.x * THREADS + threadIdx.x;
    int edge = 0, once = 0;
    if (s < slots) {
        const u64 k = keys[s];
        if (k != NO_KEY) {
            const int a = (int)(k >> 32), b = (int)(unsigned)k;
            edge = 1;
            atomicAdd(degree + a, 1);
            atomicAdd(degree + b, 1);
            if (occ[s] == 1) {
                once = 1;
                mark_or(mark, a, BOUNDARY);
                mark_or(mark, b, BOUNDARY);
            }
        }
    }
    const long long edges = block_sum<THREADS, long long>(edge, lds4), boundary = block_sum<THREADS, long long>(once, lds4);
    if (threadIdx.x == 0) {
        if (edges) atomicAdd(totals, (u64)edges);
        if (boundary) atomicAdd(totals + 1, (u64)boundary);
    }
}

__global__ __launch_bounds__(THREADS) void st_block_sums(const int* __restrict__ degree, long long n_v, long long* __restrict__ sums) {
    __shared__ long long lds4[THREADS / 64];
    const long long base = (long long)blockIdx.x * BLOCK_ITEMS;
    long long acc = 0;
    for (int r = 0; r < ITERS; ++r) {
        const long long v = base + r * THREADS + threadIdx.x;
        if (v < n_v) acc += degree[v];
    }
    const long long total = block_sum<THREADS>(acc, lds4);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: exclusive int64 scan of sums[0..nb) into offsets; the total closes the row offsets
__global__ __launch_bounds__(SCAN_THREADS) void st_scan_blocks(const long long* __restrict__ sums, long long nb, long long* __restrict__ offsets,
                                                               long long* __restrict__ row_end) {
    __shared__ long long s[2][SCAN_THREADS];
    const long long total = scan_array([=](long long b) { return sums[b]; }, nb, offsets, s);
    if (threadIdx.x == 0) *row_end = total;
}

__global__ __launch_bounds__(THREADS) void st_rows(const int* __restrict__ degree, long long n_v, const long long* __restrict__ offsets,
                                                   int pin_boundary, uint8_t* __restrict__ mark, long long* __restrict__ row_start,
                                                   int* __restrict__ degree_out, uint8_t* __restrict__ flags_out, u64* totals) {
    __shared__ long long lds4[THREADS / 64];
    const long long base = (long long)blockIdx.x * BLOCK_ITEMS;
    long long carry = offsets[blockIdx.x];
    int n_free = 0, n_boundary = 0;
    for (int r = 0; r < ITERS; ++r) {                   // block-uniform loop: every thread takes part in the scan
        const long long v = base + r * THREADS + threadIdx.x;
        const int d = v < n_v ? degree[v] : 0;
        long long total;
        const long long at = carry + block_exscan<THREADS, long long>(d, total, lds4);
        carry += total;
        if (v >= n_v) continue;
        int m = mark[v] & (INSIDE | BOUNDARY);
        if ((m & INSIDE) && d > 0 && !((m & BOUNDARY) && pin_boundary)) m |= FREE;
        row_start[v] = at;
        mark[v] = (uint8_t)m;                           // this thread alone touches the byte now: st_degrees has finished
        degree_out[v] = d;
        flags_out[v] = (uint8_t)m;
        n_free += (m & FREE) != 0;
        n_boundary += (m & BOUNDARY) != 0;
    }
    const long long tf = block_sum<THREADS, long long>(n_free, lds4), tb = block_sum<THREADS, long long>(n_boundary, lds4);
    if (threadIdx.x == 0) {
        if (tf) atomicAdd(totals + 2, (u64)tf);
        if (tb) atomicAdd(totals + 3, (u64)tb);
    }
}

__global__ __launch_bounds__(THREADS) void st_fill(const u64* __restrict__ keys, u64 slots, const long long* __restrict__ row_start,
                                                   int* cursor, int* __restrict__ adj) {
    const u64 s = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (s >= slots) return;
    const u64 k = keys[s];
    if (k == NO_KEY) return;
    const int a = (int)(k >> 32), b = (int)(unsigned)k;
    // cursor[v] starts at degree[v] and is taken down once per edge of v: the positions are 0 .. degree[v] - 1 of v's row
    const int pa = atomicSub(cursor + a, 1) - 1, pb = atomicSub(cursor + b, 1) - 1;
    if (pa >= 0) adj[row_start[a] + pa] = b;
    if (pb >= 0) adj[row_start[b] + pb] = a;
}

__global__ __launch_bounds__(THREADS) void tb_state(const float* __restrict__ vertices, long long n_v, const float* __restrict__ origin,
                                                    float cell, int4* __restrict__ q0, int4* __restrict__ q1) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_v) return;
    int q[3];
    state_of(origin, cell, vertices + 3 * v, q);
    const int4 s = make_int4(q[0], q[1], q[2], 0);
    q0[v] = s;
    q1[v] = s;
}

__device__ inline int step(int q, long long sum, int degree, double f) {
    const long long D = sum - (long long)degree * (long long)q;
    const long long moved = (long long)q + (long long)rint(f * ((double)D / (double)degree));
    return (int)min(max(moved, -(long long)QMAX), (long long)QMAX);
}

__global__ __launch_bounds__(THREADS) void tb_pass(const int4* __restrict__ before, int4* __restrict__ after,
                                                   const long long* __restrict__ row_start, const int* __restrict__ adj,
                                                   const uint8_t* __restrict__ mark, long long n_v, double f) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool active = v < n_v && (mark[v] & FREE);
    long long begin = 0, end = 0;
    if (active) {
        begin = row_start[v];
        end = row_start[v + 1];
    }
    long long s0 = 0, s1 = 0, s2 = 0;
    const bool is_long = end - begin > LONG_ROW;
    if (!is_long) {
        for (long long i = begin; i < end; ++i) {
            const int4 q = before[adj[i]];
            s0 += q.x;
            s1 += q.y;
            s2 += q.z;
        }
    }
    // wave-uniform loop over the long rows of this wave (no lane has left: the shuffles below read every lane)
    u64 todo = __ballot(is_long);
    while (todo) {
        const int owner = __ffsll((long long)todo) - 1;
        const long long rb = __shfl(begin, owner, 64), re = __shfl(end, owner, 64);
        long long t0 = 0, t1 = 0, t2 = 0;
        for (long long i = rb + lane; i < re; i += 64) {
            const int4 q = before[adj[i]];
            t0 += q.x;
            t1 += q.y;
            t2 += q.z;
        }
        t0 = wave_sum(t0);
        t1 = wave_sum(t1);
        t2 = wave_sum(t2);
        if (lane == owner) {
            s0 = t0;
            s1 = t1;
            s2 = t2;
        }
        todo &= todo - 1;
    }
    if (!active) return;
    const int4 q = before[v];
    const int degree = (int)(end - begin);              // > 0: the vertex is free
    after[v] = make_int4(step(q.x, s0, degree, f), step(q.y, s1, degree, f), step(q.z, s2, degree, f), 0);
}

__global__ __launch_bounds__(THREADS) void tb_output(const float* __restrict__ vertices, long long n_v, const float* __restrict__ origin,
                                                     float cell, const uint8_t* __restrict__ mark, const int4* __restrict__ state,
                                                     float* __restrict__ out) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_v) return;
    if (mark[v] & FREE) {
        const int4 q = state[v];
        out[3 * v] = (float)((double)origin[0] + ((double)q.x / QD) * (double)cell);
        out[3 * v + 1] = (float)((double)origin[1] + ((double)q.y / QD) * (double)cell);
        out[3 * v + 2] = (float)((double)origin[2] + ((double)q.z / QD) * (double)cell);
    } else {
        const uint32_t* s = (const uint32_t*)vertices + 3 * v;
        uint32_t* d = (uint32_t*)out + 3 * v;
        d[0] = s[0];
        d[1] = s[1];
        d[2] = s[2];
    }
}

__global__ __launch_bounds__(THREADS) void nm_faces(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                    long long n_f, u64* sums) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_f) return;
    const int i[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
    const unsigned n = (unsigned)n_v;
    if (!((unsigned)i[0] < n && (unsigned)i[1] < n && (unsigned)i[2] < n)) return;
    double p[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) p[j][k] = (double)vertices[3 * (long long)i[j] + k];
    const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
    const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
    const double c[3] = {e1y * e2z - e1z * e2y, e1z * e2x - e1x * e2z, e1x * e2y - e1y * e2x};
    const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    if (!(len > 0.0)) return;                           // false for NaN
    const double u[3] = {c[0] / len, c[1] / len, c[2] / len};
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    if (!(fabs(u[0]) < inf && fabs(u[1]) < inf && fabs(u[2]) < inf)) return;
    long long add[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) add[k] = (long long)rint(u[k] * NQ);
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (add[k]) atomicAdd(sums + 3 * (long long)i[j] + k, (u64)add[k]);
}

__global__ __launch_bounds__(THREADS) void nm_finish(const long long* __restrict__ sums, long long n_v, float* __restrict__ normal) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (v >= n_v) return;
    const double n0 = (double)sums[3 * v], n1 = (double)sums[3 * v + 1], n2 = (double)sums[3 * v + 2];
    const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    normal[3 * v] = len == 0.0 ? 0.f : (float)(n0 / len);
    normal[3 * v + 1] = len == 0.0 ? 0.f : (float)(n1 / len);
    normal[3 * v + 2] = len == 0.0 ? 0.f : (float)(n2 / len);
}

// the power of two >= 6 n_f (twice the 3 n_f sides a mesh can have), at least 64
inline size_t table_slots(long long n_f) {
    size_t t = 64;
    while (t < 6 * (size_t)n_f) t <<= 1;
    return t;
}

struct Layout {
    size_t q0, q1, row_start, cursor, mark, clear_end, block_sums, block_offsets, normal_sums, keys, occ, adj, total;
    size_t slots;
    long long nb;
};

inline Layout layout(long long n_v, long long n_f) {
    Layout l;
    l.slots = table_slots(n_f);
    l.nb = n_v ? blocks_of(n_v, BLOCK_ITEMS) : 1;
    l.q0 = 0;
    l.q1 = l.q0 + align256((size_t)n_v * 16);
    l.row_start = l.q1 + align256((size_t)n_v * 16);
    l.cursor = l.row_start + align256(((size_t)n_v + 1) * 8);
    l.mark = l.cursor + align256((size_t)n_v * 4);       // cursor and mark are cleared together
    l.clear_end = l.mark + align256((size_t)n_v);
    l.block_sums = l.clear_end;
    l.block_offsets = l.block_sums + align256((size_t)l.nb * 8);
    l.normal_sums = l.block_offsets + align256((size_t)l.nb * 8);
    l.keys = l.normal_sums + align256((size_t)n_v * 24);
    l.occ = l.keys + l.slots * 8;
    l.adj = l.occ + l.slots * 4;
    l.total = l.adj + align256((size_t)n_f * 24);
    return l;
}

inline bool factor_ok(float f) { return f >= -1.f && f <= 1.f; }          // false for NaN

}  // namespace

NGP_API int ngp_meshsmooth_abi_version(void) { return 1; }

NGP_API const char* ngp_meshsmooth_build_arch(void) { return "gfx950"; }

NGP_API size_t ngp_meshsmooth_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    if (!sizes_ok(n_vertices, n_faces)) return 0;
    return layout(n_vertices, n_faces).total;
}

NGP_API int ngp_meshsmooth_topology(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, const float* origin,
                                    float cell, int pin_boundary, void* workspace, size_t workspace_bytes, int32_t* degree, uint8_t* flags,
                                    int64_t* totals, void* stream) {
    if (n_vertices < 0 || n_faces < 0 || !cell_ok(cell)) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (n_vertices == 0) return 0;
    if (!vertices || !origin || !workspace || !degree || !flags || !totals || (n_faces > 0 && !faces)) return NGP_EINVAL;
    const Layout l = layout(n_vertices, n_faces);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const long long n_v = n_vertices, n_f = n_faces;
    u64* keys = (u64*)(ws + l.keys);
    int* occ = (int*)(ws + l.occ);
    int* cursor = (int*)(ws + l.cursor);
    uint8_t* mark = (uint8_t*)(ws + l.mark);
    long long* row_start = (long long*)(ws + l.row_start);
    hipError_t e = hipMemsetAsync(keys, 0xFF, l.slots * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(occ, 0, l.slots * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(cursor, 0, l.clear_end - l.cursor, s);
    if (e == hipSuccess) e = hipMemsetAsync(totals, 0, 32, s);
    if (e != hipSuccess) return (int)e;
    const unsigned vb = (unsigned)blocks_of(n_v, THREADS), sb = (unsigned)blocks_of((long long)l.slots, THREADS);
    hipLaunchKernelGGL(st_inside, dim3(vb), dim3(THREADS), 0, s, vertices, n_v, origin, cell, mark);
    if (n_f) {
        hipLaunchKernelGGL(st_insert, dim3((unsigned)blocks_of(n_f, THREADS)), dim3(THREADS), 0, s, faces, n_v, n_f, (const uint8_t*)mark, keys, occ,
                           (u64)l.slots);
        hipLaunchKernelGGL(st_degrees, dim3(sb), dim3(THREADS), 0, s, (const u64*)keys, (const int*)occ, (u64)l.slots, cursor, mark, (u64*)totals);
    }
    hipLaunchKernelGGL(st_block_sums, dim3((unsigned)l.nb), dim3(THREADS), 0, s, (const int*)cursor, n_v, (long long*)(ws + l.block_sums));
    hipLaunchKernelGGL(st_scan_blocks, dim3(1), dim3(SCAN_THREADS), 0, s, (const long long*)(ws + l.block_sums), l.nb,
                       (long long*)(ws + l.block_offsets), row_start + n_v);
    hipLaunchKernelGGL(st_rows, dim3((unsigned)l.nb), dim3(THREADS), 0, s, (const int*)cursor, n_v, (const long long*)(ws + l.block_offsets),
                       pin_boundary, mark, row_start, degree, flags, (u64*)totals);
    if (n_f)
        hipLaunchKernelGGL(st_fill, dim3(sb), dim3(THREADS), 0, s, (const u64*)keys, (u64)l.slots, (const long long*)row_start, cursor,
                           (int*)(ws + l.adj));
    return launched();
}

NGP_API int ngp_meshsmooth_taubin(const float* vertices, int64_t n_vertices, int64_t n_faces, const float* origin, float cell, int pairs,
                                  float lambda, float mu, void* workspace, size_t workspace_bytes, float* vertices_out, void* stream) {
    if (n_vertices < 0 || n_faces < 0 || !cell_ok(cell) || pairs < 1 || !factor_ok(lambda) || !factor_ok(mu)) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (n_vertices == 0) return 0;
    if (!vertices || !origin || !workspace || !vertices_out) return NGP_EINVAL;
    const Layout l = layout(n_vertices, n_faces);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const long long n_v = n_vertices;
    int4* q[2] = {(int4*)(ws + l.q0), (int4*)(ws + l.q1)};
    const long long* row_start = (const long long*)(ws + l.row_start);
    const int* adj = (const int*)(ws + l.adj);
    const uint8_t* mark = (const uint8_t*)(ws + l.mark);
    const unsigned vb = (unsigned)blocks_of(n_v, THREADS);
    hipLaunchKernelGGL(tb_state, dim3(vb), dim3(THREADS), 0, s, vertices, n_v, origin, cell, q[0], q[1]);
    for (int p = 0; p < pairs; ++p) {
        hipLaunchKernelGGL(tb_pass, dim3(vb), dim3(THREADS), 0, s, (const int4*)q[0], q[1], row_start, adj, mark, n_v, (double)lambda);
        hipLaunchKernelGGL(tb_pass, dim3(vb), dim3(THREADS), 0, s, (const int4*)q[1], q[0], row_start, adj, mark, n_v, (double)mu);
    }
    hipLaunchKernelGGL(tb_output, dim3(vb), dim3(THREADS), 0, s, vertices, n_v, origin, cell, mark, (const int4*)q[0], vertices_out);
    return launched();
}

NGP_API int ngp_meshsmooth_normals(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, void* workspace,
                                   size_t workspace_bytes, float* normals_out, void* stream) {
    if (n_vertices < 0 || n_faces < 0) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (n_vertices == 0) return 0;
    if (!vertices || !workspace || !normals_out || (n_faces > 0 && !faces)) return NGP_EINVAL;
    const Layout l = layout(n_vertices, n_faces);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const long long n_v = n_vertices, n_f = n_faces;
    u64* sums = (u64*)(ws + l.normal_sums);
    const hipError_t e = hipMemsetAsync(sums, 0, (size_t)n_v * 24, s);
    if (e != hipSuccess) return (int)e;
    if (n_f)
        hipLaunchKernelGGL(nm_faces, dim3((unsigned)blocks_of(n_f, THREADS)), dim3(THREADS), 0, s, vertices, faces, n_v, n_f, sums);
    hipLaunchKernelGGL(nm_finish, dim3((unsigned)blocks_of(n_v, THREADS)), dim3(THREADS), 0, s, (const long long*)sums, n_v, normals_out);
    return launched();
}
