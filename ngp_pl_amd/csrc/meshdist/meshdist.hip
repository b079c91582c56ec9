// libngp_meshdist.so: surface samples of a mesh, the nearest face of a target mesh for every query point through a uniform grid, and
// the weighted distance statistics (C ABI, the exact rule and the derivation of the slack: include/ngp_meshdist.h).  Compiled with
// -ffp-contract=off: every f32 expression below is the header's, operation by operation.
//
//   face_counts     one thread per face: k * k (rule 1), 0 for a face that is not usable.
//   block_sums / scan_block_sums / offsets   the integer exclusive scan shared by the sampler (int64 offsets per face) and the grid
//                   (uint32 list starts per cell): 256 threads x 8 elements per workgroup, the workgroup sums scanned by one workgroup
//                   (the sums and scans of ../mesh_scan.h).
//   emit_samples    one thread per sample: a binary search of the face offsets, then rule 1.  Writes are coalesced whatever k is.
//   bin_faces<FILL> one thread per face over the cells of its padded index box: an integer atomic per cell, the count in pass 1 and
//                   the slot in pass 2.
//   query           one query per lane.  Samples come in face order and marching cubes emits faces in lattice order, so the 64 lanes
//                   of a wave walk neighbouring cells and mostly the same lists: the list and vertex loads of a wave hit the same
//                   lines.  The walk, the closest point and the grid's cells are ../mesh_nearest.h, shared with
//                   libngp_meshnormal.so; here every candidate is accepted.
//   stats / stats_finish   the two-stage f64 sums of rule 4, as libngp_metrics.so does them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../../include/ngp_meshdist.h"

namespace {

#include "../mesh_host.h"
#include "../mesh_scan.h"

constexpr int THREADS = 256;
constexpr int SCAN_ITEMS = NGP_MESHDIST_SCAN_BLOCK / THREADS;        // 8
constexpr int K_MAX = NGP_MESHDIST_K_MAX;
constexpr int NT = NGP_MESHDIST_MAX_THRESHOLDS;
constexpr int NOUT = NGP_MESHDIST_STATS_OUTPUTS;
constexpr int STATS_MAX_BLOCKS = NGP_MESHDIST_STATS_MAX_BLOCKS;
constexpr float SLACK_FACTOR = (float)NGP_MESHDIST_SLACK_ULPS * 0x1p-23f;
constexpr int MAX_AXIS = NGP_MESHDIST_MAX_AXIS;
constexpr long long MAX_CELLS = NGP_MESHDIST_MAX_CELLS;
static_assert(NGP_MESHDIST_SCAN_BLOCK % THREADS == 0 && NOUT == 6 + NT, "header constants");

#include "../mesh_nearest.h"

// rule 1: k
__device__ inline int subdivision(V3 a, V3 b, V3 c, float spacing) {
    const V3 ab = sub(b, a), ac = sub(c, a), bc = sub(c, b);
    const float longest = fmaxf(fmaxf(sqrtf(dot(ab, ab)), sqrtf(dot(ac, ac))), sqrtf(dot(bc, bc)));
    const float q = ceilf(longest / spacing);
    if (!(q >= 1.0f)) return 1;
    if (q >= (float)K_MAX) return K_MAX;
    return (int)q;
}

__device__ inline int isqrt_small(int s) {                  // s < 2^22
    int r = (int)sqrtf((float)s);
    while (r * r > s) --r;
    while ((r + 1) * (r + 1) <= s) ++r;
    return r;
}

// ---- the sampler

__global__ __launch_bounds__(THREADS) void face_counts(const float* __restrict__ v, const int32_t* __restrict__ f, int n_v, int n_f, float spacing,
                                                       int32_t* __restrict__ counts) {
    const long long face = (long long)blockIdx.x * THREADS + threadIdx.x;      // 64-bit: the last block may pass INT32_MAX
    if (face >= n_f) return;
    V3 a, b, c;
    int n = 0;
    if (load_face(v, f, n_v, face, a, b, c)) {
        const int k = subdivision(a, b, c, spacing);
        n = k * k;
    }
    counts[face] = n;
}

// ---- the scan: counts (n) -> exclusive offsets (n + 1), the last one the total

__global__ __launch_bounds__(THREADS) void block_sums(const int32_t* __restrict__ counts, long long n, long long* __restrict__ bsum) {
    __shared__ long long lds4[THREADS / 64];
    const long long base = (long long)blockIdx.x * NGP_MESHDIST_SCAN_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
    long long s = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j)
        if (base + j < n) s += (uint32_t)counts[base + j];
    const long long total = block_sum<THREADS>(s, lds4);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum becomes its own exclusive scan, *total the sum
__global__ __launch_bounds__(SCAN_THREADS) void scan_block_sums(long long* bsum, long long nb, long long* __restrict__ total) {
    __shared__ long long s[2][SCAN_THREADS];
    const long long sum = scan_array([=](long long b) { return bsum[b]; }, nb, bsum, s);
    if (threadIdx.x == 0) *total = sum;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void offsets(const int32_t* __restrict__ counts, long long n, const long long* __restrict__ bsum,
                                                   T* __restrict__ out) {
    __shared__ long long lds4[THREADS / 64];
    const long long base = (long long)blockIdx.x * NGP_MESHDIST_SCAN_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
    long long own = 0;
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j)
        if (base + j < n) own += (uint32_t)counts[base + j];
    long long total;
    long long at = bsum[blockIdx.x] + block_exscan<THREADS>(own, total, lds4);
#pragma unroll
    for (int j = 0; j < SCAN_ITEMS; ++j) {
        if (base + j < n) {
            out[base + j] = (T)at;
            at += (uint32_t)counts[base + j];
        }
        if (base + j == n - 1) out[n] = (T)at;             // the total closes the last list
    }
}

__global__ __launch_bounds__(THREADS) void emit_samples(const float* __restrict__ v, const int32_t* __restrict__ f, int n_v, int n_f, float spacing,
                                                        const long long* __restrict__ start, int n_samples, float* __restrict__ points,
                                                        float* __restrict__ weights, int32_t* __restrict__ face_ids) {
    const long long g = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (g >= n_samples) return;
    int lo = 0, hi = n_f - 1;                               // the last face with start[face] <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const int face = lo;
    const int s = (int)(g - start[face]);
    V3 a, b, c;
    if (!load_face(v, f, n_v, face, a, b, c)) return;      // not reached: such a face has no samples
    const int k = subdivision(a, b, c, spacing);
    const int r = isqrt_small(s), col = s - r * r, t = col >> 1;
    int i, j, l;
    if ((col & 1) == 0) {
        i = 3 * (k - r) - 2, j = 3 * (r - t) + 1, l = 3 * t + 1;
    } else {
        i = 3 * (k - r) - 1, j = 3 * (r - t) - 1, l = 3 * t + 2;
    }
    const float fi = (float)i, fj = (float)j, fl = (float)l, den = (float)(3 * k);
    points[3 * g] = ((fi * a.x + fj * b.x) + fl * c.x) / den;
    points[3 * g + 1] = ((fi * a.y + fj * b.y) + fl * c.y) / den;
    points[3 * g + 2] = ((fi * a.z + fj * b.z) + fl * c.z) / den;
    const V3 ab = sub(b, a), ac = sub(c, a);
    const V3 n = {ab.y * ac.z - ab.z * ac.y, ab.z * ac.x - ab.x * ac.z, ab.x * ac.y - ab.y * ac.x};
    weights[g] = (0.5f * sqrtf(dot(n, n))) / (float)(k * k);
    face_ids[g] = face;
}

// ---- the grid

// pass 1 (FILL = false): counts[cell] += 1; pass 2: entries[start[cell] + cursor[cell]++] = face
template <bool FILL>
__global__ __launch_bounds__(THREADS) void bin_faces(const float* __restrict__ v, const int32_t* __restrict__ f, int n_v, int n_f, Grid g,
                                                     uint32_t* __restrict__ counts, const uint32_t* __restrict__ start, int32_t* __restrict__ entries,
                                                     int n_entries) {
    const long long gid = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (gid >= n_f) return;
    const int face = (int)gid;
    V3 a, b, c;
    if (!load_face(v, f, n_v, face, a, b, c)) return;
    const float m = fmaxf(g.m_grid, fmaxf(fmaxf(absmax3(a), absmax3(b)), absmax3(c)));
    const float s = SLACK_FACTOR * m;
    const int x0 = cell_of(fminf(fminf(a.x, b.x), c.x) - s, g.ox, g.cell, g.nx), x1 = cell_of(fmaxf(fmaxf(a.x, b.x), c.x) + s, g.ox, g.cell, g.nx);
    const int y0 = cell_of(fminf(fminf(a.y, b.y), c.y) - s, g.oy, g.cell, g.ny), y1 = cell_of(fmaxf(fmaxf(a.y, b.y), c.y) + s, g.oy, g.cell, g.ny);
    const int z0 = cell_of(fminf(fminf(a.z, b.z), c.z) - s, g.oz, g.cell, g.nz), z1 = cell_of(fmaxf(fmaxf(a.z, b.z), c.z) + s, g.oz, g.cell, g.nz);
    for (int z = z0; z <= z1; ++z)
        for (int y = y0; y <= y1; ++y)
            for (int x = x0; x <= x1; ++x) {
                const long long cell = ((long long)z * g.ny + y) * g.nx + x;
                const uint32_t slot = atomicAdd(&counts[cell], 1u);
                if (FILL) {
                    const uint32_t at = start[cell] + slot;
                    if (at < (uint32_t)n_entries) entries[at] = face;   // never false after pass 1 with the same arguments
                }
            }
}

__global__ __launch_bounds__(THREADS) void query(const float* __restrict__ points, int n_points, const float* __restrict__ v,
                                                 const int32_t* __restrict__ f, int n_v, int n_f, Grid g, float max_dist, float max_d2,
                                                 const uint32_t* __restrict__ start, const int32_t* __restrict__ entries, int n_entries,
                                                 float* __restrict__ out_d2, int32_t* __restrict__ out_face, float* __restrict__ closest,
                                                 uint32_t* __restrict__ debug) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_points) return;
    const V3 p = load3(points, i);
    unsigned long long best = ~0ull;                        // bits(d2) << 32 | face
    uint32_t shells = 0, evaluated = 0;
    if (finite3(p)) best = nearest_face(p, AcceptAll{}, v, f, n_v, n_f, g, SLACK_FACTOR, max_dist, start, entries, n_entries, &shells, &evaluated);
    float d2 = __uint_as_float((uint32_t)(best >> 32));
    int face = (int)(uint32_t)best;
    const float nan = __uint_as_float(0x7FC00000u);
    V3 q = {nan, nan, nan};
    if (best == ~0ull || d2 > max_d2) {
        d2 = __uint_as_float(0x7F800000u);
        face = -1;
    } else if (closest) {
        V3 a, b, c;
        load_face(v, f, n_v, face, a, b, c);
        q = closest_point(p, a, b, c);
    }
    out_d2[i] = d2;
    out_face[i] = face;
    if (closest) {
        closest[3 * i] = q.x;
        closest[3 * i + 1] = q.y;
        closest[3 * i + 2] = q.z;
    }
    if (debug) {
        debug[2 * i] = shells;
        debug[2 * i + 1] = evaluated;
    }
}

// ---- the statistics

struct Thresholds {
    float t2[NT];                                           // tau * tau; -1 past n_thresholds (no d2 is <= -1)
};

__device__ inline double wave_add(double s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    return s;
}

__device__ inline double wave_max(double s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s = fmax(s, __shfl_down(s, off));
    return s;
}

// slot 3 is a maximum, the others sums: lane 0 of every wave -> LDS, thread 0 combines the waves in index order
template <int WAVES>
__device__ inline void block_store(double val, int slot, double* lds, double* __restrict__ out) {
    val = slot == 3 ? wave_max(val) : wave_add(val);
    const int tid = threadIdx.x;
    __syncthreads();
    if ((tid & 63) == 0) lds[tid >> 6] = val;
    __syncthreads();
    if (tid == 0) {
        double a = lds[0];
#pragma unroll
        for (int k = 1; k < WAVES; ++k) a = slot == 3 ? fmax(a, lds[k]) : a + lds[k];
        out[slot] = a;
    }
}

__global__ __launch_bounds__(THREADS) void stats(const float* __restrict__ d2, const int32_t* __restrict__ face, const float* __restrict__ weights,
                                                 int n, Thresholds th, double* __restrict__ partials) {
    __shared__ double lds[THREADS / 64];
    double sw = 0.0, swd = 0.0, swd2 = 0.0, mx = 0.0, mw = 0.0, mn = 0.0;
    double in0 = 0.0, in1 = 0.0, in2 = 0.0, in3 = 0.0, in4 = 0.0, in5 = 0.0, in6 = 0.0, in7 = 0.0;
    const long long stride = (long long)gridDim.x * THREADS;
    for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < n; i += stride) {
        const double w = (double)weights[i];
        if (face[i] >= 0) {
            const float x = d2[i];
            const float d = sqrtf(x);
            sw += w;
            swd += w * (double)d;
            swd2 += w * (double)x;
            mx = fmax(mx, (double)d);
            if (x <= th.t2[0]) in0 += w;
            if (x <= th.t2[1]) in1 += w;
            if (x <= th.t2[2]) in2 += w;
            if (x <= th.t2[3]) in3 += w;
            if (x <= th.t2[4]) in4 += w;
            if (x <= th.t2[5]) in5 += w;
            if (x <= th.t2[6]) in6 += w;
            if (x <= th.t2[7]) in7 += w;
        } else {
            mw += w;
            mn += 1.0;
        }
    }
    double* out = partials + (long long)blockIdx.x * NOUT;
    constexpr int W = THREADS / 64;
    block_store<W>(sw, 0, lds, out);
    block_store<W>(swd, 1, lds, out);
    block_store<W>(swd2, 2, lds, out);
    block_store<W>(mx, 3, lds, out);
    block_store<W>(mw, 4, lds, out);
    block_store<W>(mn, 5, lds, out);
    block_store<W>(in0, 6, lds, out);
    block_store<W>(in1, 7, lds, out);
    block_store<W>(in2, 8, lds, out);
    block_store<W>(in3, 9, lds, out);
    block_store<W>(in4, 10, lds, out);
    block_store<W>(in5, 11, lds, out);
    block_store<W>(in6, 12, lds, out);
    block_store<W>(in7, 13, lds, out);
}

// one wave: output `slot` per iteration, lane l the partials l, l + 64, ... in index order, then the tree
__global__ __launch_bounds__(64) void stats_finish(const double* __restrict__ partials, int blocks, double* __restrict__ out) {
    for (int slot = 0; slot < NOUT; ++slot) {
        double s = 0.0;
        for (int j = threadIdx.x; j < blocks; j += 64) {
            const double x = partials[(long long)j * NOUT + slot];
            s = slot == 3 ? fmax(s, x) : s + x;
        }
        s = slot == 3 ? wave_max(s) : wave_add(s);
        if (threadIdx.x == 0) out[slot] = s;
    }
}

// ---- host side

inline long long scan_blocks(long long n) { return (n + NGP_MESHDIST_SCAN_BLOCK - 1) / NGP_MESHDIST_SCAN_BLOCK; }
inline size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

// the layout of the sampler's workspace: offsets (n + 1) i64, block sums i64, counts (n) i32
struct SampleWs {
    long long* start;
    long long* bsum;
    int32_t* counts;
};
inline SampleWs sample_ws(void* ws, long long n_f) {
    SampleWs w;
    w.start = (long long*)ws;
    w.bsum = w.start + (n_f + 1);
    w.counts = (int32_t*)(w.bsum + scan_blocks(n_f));
    return w;
}

// the layout of the grid's workspace: block sums i64, list starts (cells + 1) u32, counts / cursors (cells) u32
struct GridWs {
    long long* bsum;
    uint32_t* start;
    uint32_t* counts;
};
inline GridWs grid_ws(const void* ws, long long cells) {
    GridWs w;
    w.bsum = (long long*)ws;
    w.start = (uint32_t*)(w.bsum + scan_blocks(cells));
    w.counts = w.start + (cells + 1);
    return w;
}

// the shared checks of the three grid entry points: 0, NGP_EINVAL or NGP_ERANGE; fills g
inline int check_grid(const void* vertices, const void* faces, int64_t n_vertices, int64_t n_faces, const float* origin, float cell, int nx,
                      int ny, int nz, const void* workspace, size_t workspace_bytes, Grid& g) {
    if (n_vertices < 0 || n_faces < 0 || !origin || !workspace) return NGP_EINVAL;
    if ((!vertices && n_vertices > 0) || (!faces && n_faces > 0)) return NGP_EINVAL;
    const float m = grid_magnitude(origin, cell, nx, ny, nz, MAX_AXIS, MAX_CELLS);
    if (m < 0.0f) return NGP_EINVAL;
    if (cell < (float)NGP_MESHDIST_MIN_CELL_SLACKS * (SLACK_FACTOR * m)) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (workspace_bytes < ngp_meshdist_grid_workspace_bytes(nx, ny, nz) || ((uintptr_t)workspace & 7) != 0) return NGP_EINVAL;
    g = Grid{origin[0], origin[1], origin[2], cell, m, nx, ny, nz};
    return 0;
}

inline int check_sampler(const void* vertices, const void* faces, int64_t n_vertices, int64_t n_faces, float spacing, const void* workspace,
                         size_t workspace_bytes) {
    if (n_vertices < 0 || n_faces < 0 || !(spacing > 0.0f) || !isfinite(spacing)) return NGP_EINVAL;
    if ((!vertices && n_vertices > 0) || (!faces && n_faces > 0) || (!workspace && n_faces > 0)) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (n_faces > 0 && (workspace_bytes < ngp_meshdist_sample_workspace_bytes(n_faces) || ((uintptr_t)workspace & 7) != 0)) return NGP_EINVAL;
    return 0;
}

}  // namespace

NGP_API int ngp_meshdist_abi_version(void) { return 1; }

NGP_API const char* ngp_meshdist_build_arch(void) { return "gfx950"; }

NGP_API int ngp_meshdist_slack(const float* origin, float cell, int nx, int ny, int nz, float* slack, float* min_cell) {
    if (!slack || !min_cell) return NGP_EINVAL;
    const float m = grid_magnitude(origin, cell, nx, ny, nz, MAX_AXIS, MAX_CELLS);
    if (m < 0.0f) return NGP_EINVAL;
    *slack = SLACK_FACTOR * m;
    *min_cell = (float)NGP_MESHDIST_MIN_CELL_SLACKS * (SLACK_FACTOR * m);
    return 0;
}

NGP_API size_t ngp_meshdist_sample_workspace_bytes(int64_t n_faces) {
    if (n_faces < 1 || n_faces > INT32_MAX) return 0;
    return 8 * (size_t)(n_faces + 1) + 8 * (size_t)scan_blocks(n_faces) + align8(4 * (size_t)n_faces);
}

NGP_API int ngp_meshdist_sample_count(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float spacing,
                                      void* workspace, size_t workspace_bytes, int64_t* total, void* stream) {
    const int rc = check_sampler(vertices, faces, n_vertices, n_faces, spacing, workspace, workspace_bytes);
    if (rc) return rc;
    if (!total) return NGP_EINVAL;
    if (n_faces == 0) return 0;
    const SampleWs w = sample_ws(workspace, n_faces);
    const long long nb = scan_blocks(n_faces);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(face_counts, dim3((unsigned)((n_faces + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, vertices, faces, (int)n_vertices,
                       (int)n_faces, spacing, w.counts);
    hipLaunchKernelGGL(block_sums, dim3((unsigned)nb), dim3(THREADS), 0, s, (const int32_t*)w.counts, (long long)n_faces, w.bsum);
    hipLaunchKernelGGL(scan_block_sums, dim3(1), dim3(SCAN_THREADS), 0, s, w.bsum, nb, (long long*)total);
    hipLaunchKernelGGL(offsets<long long>, dim3((unsigned)nb), dim3(THREADS), 0, s, (const int32_t*)w.counts, (long long)n_faces,
                       (const long long*)w.bsum, w.start);
    return launched();
}

NGP_API int ngp_meshdist_sample_emit(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float spacing,
                                     void* workspace, size_t workspace_bytes, int64_t n_samples, float* points, float* weights,
                                     int32_t* face_ids, void* stream) {
    const int rc = check_sampler(vertices, faces, n_vertices, n_faces, spacing, workspace, workspace_bytes);
    if (rc) return rc;
    if (n_samples < 0 || (n_samples > 0 && (!points || !weights || !face_ids || n_faces == 0))) return NGP_EINVAL;
    if (n_samples > INT32_MAX) return NGP_ERANGE;
    if (n_samples == 0) return 0;
    const SampleWs w = sample_ws(workspace, n_faces);
    hipLaunchKernelGGL(emit_samples, dim3((unsigned)((n_samples + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, vertices, faces,
                       (int)n_vertices, (int)n_faces, spacing, (const long long*)w.start, (int)n_samples, points, weights, face_ids);
    return launched();
}

NGP_API size_t ngp_meshdist_grid_workspace_bytes(int nx, int ny, int nz) {
    if (!axes_ok(nx, ny, nz, MAX_AXIS, MAX_CELLS)) return 0;
    const long long cells = (long long)nx * ny * nz;
    return 8 * (size_t)scan_blocks(cells) + 4 * (size_t)(cells + 1) + 4 * (size_t)cells;
}

NGP_API int ngp_meshdist_grid_count(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, const float* origin,
                                    float cell, int nx, int ny, int nz, void* workspace, size_t workspace_bytes, int64_t* total,
                                    void* stream) {
    Grid g;
    const int rc = check_grid(vertices, faces, n_vertices, n_faces, origin, cell, nx, ny, nz, workspace, workspace_bytes, g);
    if (rc) return rc;
    if (!total) return NGP_EINVAL;
    const long long cells = (long long)nx * ny * nz, nb = scan_blocks(cells);
    const GridWs w = grid_ws(workspace, cells);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t cleared = hipMemsetAsync(w.counts, 0, 4 * (size_t)cells, s);
    if (cleared != hipSuccess) return (int)cleared;
    if (n_faces > 0)
        hipLaunchKernelGGL(bin_faces<false>, dim3((unsigned)((n_faces + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, vertices, faces,
                           (int)n_vertices, (int)n_faces, g, w.counts, (const uint32_t*)nullptr, (int32_t*)nullptr, 0);
    hipLaunchKernelGGL(block_sums, dim3((unsigned)nb), dim3(THREADS), 0, s, (const int32_t*)w.counts, cells, w.bsum);
    hipLaunchKernelGGL(scan_block_sums, dim3(1), dim3(SCAN_THREADS), 0, s, w.bsum, nb, (long long*)total);
    hipLaunchKernelGGL(offsets<uint32_t>, dim3((unsigned)nb), dim3(THREADS), 0, s, (const int32_t*)w.counts, cells, (const long long*)w.bsum,
                       w.start);
    return launched();
}

NGP_API int ngp_meshdist_grid_fill(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, const float* origin,
                                   float cell, int nx, int ny, int nz, void* workspace, size_t workspace_bytes, int64_t n_entries,
                                   int32_t* entries, void* stream) {
    Grid g;
    const int rc = check_grid(vertices, faces, n_vertices, n_faces, origin, cell, nx, ny, nz, workspace, workspace_bytes, g);
    if (rc) return rc;
    if (n_entries < 0 || (n_entries > 0 && !entries)) return NGP_EINVAL;
    if (n_entries > INT32_MAX) return NGP_ERANGE;
    if (n_entries == 0 || n_faces == 0) return 0;
    const long long cells = (long long)nx * ny * nz;
    const GridWs w = grid_ws(workspace, cells);
    hipStream_t s = (hipStream_t)stream;
    const hipError_t cleared = hipMemsetAsync(w.counts, 0, 4 * (size_t)cells, s);
    if (cleared != hipSuccess) return (int)cleared;
    hipLaunchKernelGGL(bin_faces<true>, dim3((unsigned)((n_faces + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, vertices, faces, (int)n_vertices,
                       (int)n_faces, g, w.counts, (const uint32_t*)w.start, entries, (int)n_entries);
    return launched();
}

NGP_API int ngp_meshdist_query(const float* points, int64_t n_points, const float* vertices, const int32_t* faces, int64_t n_vertices,
                               int64_t n_faces, const float* origin, float cell, int nx, int ny, int nz, float max_dist,
                               const void* workspace, size_t workspace_bytes, const int32_t* entries, int64_t n_entries, float* d2,
                               int32_t* face, float* closest, uint32_t* debug, void* stream) {
    Grid g;
    const int rc = check_grid(vertices, faces, n_vertices, n_faces, origin, cell, nx, ny, nz, workspace, workspace_bytes, g);
    if (rc) return rc;
    if (n_points < 0 || n_entries < 0 || !(max_dist >= 0.0f)) return NGP_EINVAL;
    if (n_points > 0 && (!points || !d2 || !face)) return NGP_EINVAL;
    if (n_entries > 0 && !entries) return NGP_EINVAL;
    if (n_points > INT32_MAX || n_entries > INT32_MAX) return NGP_ERANGE;
    if (n_points == 0) return 0;
    const GridWs w = grid_ws(workspace, (long long)nx * ny * nz);
    hipLaunchKernelGGL(query, dim3((unsigned)((n_points + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, points, (int)n_points,
                       vertices, faces, (int)n_vertices, (int)n_faces, g, max_dist, max_dist * max_dist, (const uint32_t*)w.start, entries,
                       (int)n_entries, d2, face, closest, debug);
    return launched();
}

NGP_API size_t ngp_meshdist_stats_workspace_bytes(int64_t n) {
    if (n < 1 || n > INT32_MAX) return 0;
    const long long blocks = (n + THREADS - 1) / THREADS;
    return (size_t)NOUT * 8 * (size_t)(blocks < STATS_MAX_BLOCKS ? blocks : STATS_MAX_BLOCKS);
}

NGP_API int ngp_meshdist_stats(const float* d2, const int32_t* face, const float* weights, int64_t n, const float* thresholds,
                               int n_thresholds, void* workspace, size_t workspace_bytes, double* out, void* stream) {
    if (!d2 || !face || !weights || !workspace || !out) return NGP_EINVAL;
    if (n < 1 || n_thresholds < 0 || n_thresholds > NT || (n_thresholds > 0 && !thresholds)) return NGP_EINVAL;
    if (n > INT32_MAX) return NGP_ERANGE;
    Thresholds th;
    for (int t = 0; t < NT; ++t) {
        th.t2[t] = -1.0f;
        if (t < n_thresholds) {
            if (!(thresholds[t] >= 0.0f)) return NGP_EINVAL;
            th.t2[t] = thresholds[t] * thresholds[t];
        }
    }
    const size_t need = ngp_meshdist_stats_workspace_bytes(n);
    if (workspace_bytes < need || ((uintptr_t)workspace & 7) != 0) return NGP_EINVAL;
    const int blocks = (int)(need / ((size_t)NOUT * 8));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(stats, dim3((unsigned)blocks), dim3(THREADS), 0, s, d2, face, weights, (int)n, th, (double*)workspace);
    hipLaunchKernelGGL(stats_finish, dim3(1), dim3(64), 0, s, (const double*)workspace, blocks, out);
    return launched();
}
