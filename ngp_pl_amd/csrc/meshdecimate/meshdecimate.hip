// libngp_meshdecimate.so: decimation of a mesh by rounds of independent half-edge collapses (C ABI and the exact rule:
// include/ngp_meshdecimate.h).  Compiled with -ffp-contract=off: every f64 expression below is the header's, operation by operation.
//
// ngp_meshdecimate_begin:
//   md_init          one thread per face: the face, or (-1, -1, -1) when an index is out of range or repeated (DEAD).
// ngp_meshdecimate_round, on the caller's stream:
//   clear            degrees, fill cursors and counters to 0, claim words to NONE;
//   md_count         one thread per face: the corners per vertex, the number of current faces;
//   md_alloc         one thread per vertex: a row of `degree` slots, by a wave scan and one add per wave (rows land in any order:
//                    they feed integer sums and boolean results only);
//   md_fill          one thread per corner's face: the corner's number 3 f + j into its vertex's row;
//   md_eval          one wave per vertex u, lane k holds corner k = (u, a, b) with the positions of a and b: the fan test with
//                    shuffles over the corners, then for every target v = a_i in turn the link condition and the duplicate test
//                    against v's row (read through scalar registers: v is wave-uniform), flip, error and cost per lane, ballots
//                    and a wave sum; the best (cost, len, v); the candidate's key goes into the claim words of u and N(u);
//   md_win           one thread per candidate: all claim words of its closed one-ring hold its key; the round's totals.
// ngp_meshdecimate_apply:
//   md_select        only when fewer winners are kept than won: one workgroup, an 8-bit radix select of the n_keep-th smallest key;
//   md_rewrite       one thread per face: an applied winner among the indices becomes its target; degenerate faces die.
// ngp_meshdecimate_count / _emit: the shared order-preserving compaction of ../mesh_compact.h over the current faces.
// Integer atomics only: every output is bit-identical run to run and for any launch shape.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/ngp_meshdecimate.h"

namespace {

#include "../mesh_compact.h"

typedef unsigned long long u64;

constexpr int MAX_DEGREE = NGP_MESHDECIMATE_MAX_DEGREE;
constexpr double SD = 1048576.0;                        // the header's S
constexpr double CAP = 1125899906842624.0;              // 2^50
constexpr u64 NONE = ~0ull;
constexpr int WAVES = THREADS / 64;                     // vertices per block of md_eval
constexpr int SELECT_THREADS = 1024;

struct Counters {                                       // cleared every round
    u64 candidates, winners, faces;
    unsigned cursor;                                    // slots handed out by md_alloc
    unsigned pad;
    u64 threshold;                                      // md_rewrite applies winners with key <= threshold
};

struct Ws {
    int* faces;                                         // (F, 3) current faces
    int* rows;                                          // 3 F corner numbers, grouped by vertex
    int* degree;                                        // V                      | cleared together
    int* filled;                                        // V                      |
    Counters* counters;                                 //                        |
    u64* claim;                                         // V                      | set to NONE together
    u64* wkey;                                          // V  a winner's key      |
    u64* ckey;                                          // V  a candidate's key, NONE otherwise (md_eval writes every word)
    int* start;                                         // V
    int* target;                                        // V
    char* compact;                                      // the workspace of mesh_compact.h
    size_t zero_bytes, none_bytes, total;
};

inline Ws carve(char* base, long long n_v, long long n_f) {
    Ws w;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char* p = base + o;
        o += align256(bytes);
        return p;
    };
    w.faces = (int*)take((size_t)n_f * 12);
    w.rows = (int*)take((size_t)n_f * 12);
    const size_t z0 = o;
    w.degree = (int*)take((size_t)n_v * 4);
    w.filled = (int*)take((size_t)n_v * 4);
    w.counters = (Counters*)take(sizeof(Counters));
    w.zero_bytes = o - z0;
    const size_t n0 = o;
    w.claim = (u64*)take((size_t)n_v * 8);
    w.wkey = (u64*)take((size_t)n_v * 8);
    w.none_bytes = o - n0;
    w.ckey = (u64*)take((size_t)n_v * 8);
    w.start = (int*)take((size_t)n_v * 4);
    w.target = (int*)take((size_t)n_v * 4);
    w.compact = base + o;
    w.total = o + align256(layout(n_v, n_f).total);
    return w;
}

__device__ inline unsigned mix(unsigned u) {
    unsigned x = u * 0x9E3779B1u;
    x ^= x >> 15;
    x *= 0x85EBCA77u;
    x ^= x >> 13;
    return x;
}

// the header's code(): the cost to 24 significant bits, truncated
__device__ inline unsigned code(long long c) {
    if (c <= 0) return 0;
    const int e = 63 - __clzll(c);
    const u64 m = e >= 23 ? (u64)c >> (e - 23) : (u64)c << (23 - e);
    return ((unsigned)(e + 1) << 23) | ((unsigned)m & 0x7FFFFFu);
}

__device__ inline bool finite3(float x, float y, float z) {
    const float inf = __uint_as_float(0x7F800000u);
    return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;         // false for NaN
}

__global__ __launch_bounds__(THREADS) void md_init(const int* __restrict__ faces, long long n_v, long long n_f, int* __restrict__ cur) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_f) return;
    int v[3];
    const bool ok = load_face(faces, f, (unsigned)n_v, v) && v[0] != v[1] && v[1] != v[2] && v[0] != v[2];
    cur[3 * f] = ok ? v[0] : -1;
    cur[3 * f + 1] = ok ? v[1] : -1;
    cur[3 * f + 2] = ok ? v[2] : -1;
}

__global__ __launch_bounds__(THREADS) void md_count(const int* __restrict__ cur, long long n_f, int* degree, Counters* counters) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    const bool live = f < n_f && cur[3 * f] >= 0;
    if (live) {
        atomicAdd(degree + cur[3 * f], 1);
        atomicAdd(degree + cur[3 * f + 1], 1);
        atomicAdd(degree + cur[3 * f + 2], 1);
    }
    const u64 m = __ballot(live);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&counters->faces, (u64)__popcll(m));
}

__global__ __launch_bounds__(THREADS) void md_alloc(const int* __restrict__ degree, long long n_v, int* __restrict__ start, Counters* counters) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int d = v < n_v ? degree[v] : 0;
    const int x = wave_incscan(d);
    const int total = __shfl(x, 63, 64);
    unsigned base = 0;
    if (lane == 63 && total) base = atomicAdd(&counters->cursor, (unsigned)total);
    base = __shfl(base, 63, 64);
    if (v < n_v) start[v] = (int)base + x - d;          // the sum of all degrees is 3 * faces <= INT32_MAX
}

__global__ __launch_bounds__(THREADS) void md_fill(const int* __restrict__ cur, long long n_f, const int* __restrict__ start, int* filled,
                                                   int* __restrict__ rows) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_f || cur[3 * f] < 0) return;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int v = cur[3 * f + j];
        rows[start[v] + atomicAdd(filled + v, 1)] = (int)(3 * f + j);
    }
}

__global__ __launch_bounds__(THREADS) void md_eval(const float* __restrict__ vertices, const int* __restrict__ cur,
                                                   const int* __restrict__ degree, const int* __restrict__ start,
                                                   const int* __restrict__ rows, long long n_v, double e2, double kc, double kl,
                                                   u64* claim, u64* __restrict__ ckey, int* __restrict__ target) {
    const long long u = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (u >= n_v) return;                               // the whole wave
    const int lane = threadIdx.x & 63;
    const int d = __builtin_amdgcn_readfirstlane(degree[u]);
    u64 key = NONE;
    int tgt = -1;
    if (d >= 3 && d <= MAX_DEGREE) {
        const bool active = lane < d;
        const float pu0 = vertices[3 * u], pu1 = vertices[3 * u + 1], pu2 = vertices[3 * u + 2];
        int a = -1, b = -2;
        float pa0 = 0.f, pa1 = 0.f, pa2 = 0.f, pb0 = 0.f, pb1 = 0.f, pb2 = 0.f;
        if (active) {
            const int r = rows[start[u] + lane];
            const int f = r / 3, j = r - 3 * f;
            a = cur[3 * (size_t)f + (j + 1) % 3];
            b = cur[3 * (size_t)f + (j + 2) % 3];
            pa0 = vertices[3 * (size_t)a], pa1 = vertices[3 * (size_t)a + 1], pa2 = vertices[3 * (size_t)a + 2];
            pb0 = vertices[3 * (size_t)b], pb1 = vertices[3 * (size_t)b + 1], pb2 = vertices[3 * (size_t)b + 2];
        }
        // REMOVABLE: every a once, every b once, every b some corner's a; then one cycle of successors
        int na = 0, nb = 0, ns = 0, succ = 0;
        for (int j = 0; j < d; ++j) {
            const int aj = __shfl(a, j, 64), bj = __shfl(b, j, 64);
            na += aj == a;
            nb += bj == b;
            if (aj == b) {
                ++ns;
                succ = j;
            }
        }
        const bool mine = !active || (na == 1 && nb == 1 && ns == 1 && finite3(pa0, pa1, pa2));
        bool fan = __ballot(!mine) == 0 && finite3(pu0, pu1, pu2);
        if (fan) {
            int at = 0, steps = 0;
            do {
                at = __shfl(succ, at, 64);
                ++steps;
            } while (at != 0 && steps < d);
            fan = at == 0 && steps == d;
        }
        if (fan) {
            const double e10 = (double)pa0 - (double)pu0, e11 = (double)pa1 - (double)pu1, e12 = (double)pa2 - (double)pu2;
            const double e20 = (double)pb0 - (double)pu0, e21 = (double)pb1 - (double)pu1, e22 = (double)pb2 - (double)pu2;
            const double c0 = e11 * e22 - e12 * e21, c1 = e12 * e20 - e10 * e22, c2 = e10 * e21 - e11 * e20;
            const double ll = (c0 * c0 + c1 * c1) + c2 * c2;
            const double len = sqrt(ll);
            long long best_cost = 0, best_len = 0;
            for (int i = 0; i < d; ++i) {
                const int v = __builtin_amdgcn_readfirstlane(__shfl(a, i, 64));
                const float pv0 = __shfl(pa0, i, 64), pv1 = __shfl(pa1, i, 64), pv2 = __shfl(pa2, i, 64);
                const bool has_v = a == v || b == v;
                const double dv0 = (double)pv0 - (double)pu0, dv1 = (double)pv1 - (double)pu1, dv2 = (double)pv2 - (double)pu2;
                const double f10 = (double)pa0 - (double)pv0, f11 = (double)pa1 - (double)pv1, f12 = (double)pa2 - (double)pv2;
                const double f20 = (double)pb0 - (double)pv0, f21 = (double)pb1 - (double)pv1, f22 = (double)pb2 - (double)pv2;
                const double q0 = f11 * f22 - f12 * f21, q1 = f12 * f20 - f10 * f22, q2 = f10 * f21 - f11 * f20;
                const double dot = (c0 * q0 + c1 * q1) + c2 * q2;
                const double g = (c0 * dv0 + c1 * dv1) + c2 * dv2;
                bool ok = dot > 0.0;
                if (e2 >= 0.0) ok = ok && g * g <= e2 * ll;
                // v's row, whatever its length: which of N(u) lie in N(v), and whether a current face holds v, a, b
                const int dv = __builtin_amdgcn_readfirstlane(degree[v]), sv = __builtin_amdgcn_readfirstlane(start[v]);
                bool linked = false, dup = false;
                for (int q = 0; q < dv; ++q) {
                    const int f = __builtin_amdgcn_readfirstlane(rows[sv + q]) / 3;
                    const int x0 = cur[3 * (size_t)f], x1 = cur[3 * (size_t)f + 1], x2 = cur[3 * (size_t)f + 2];
                    const bool in_a = a == x0 || a == x1 || a == x2;
                    const bool in_b = b == x0 || b == x1 || b == x2;
                    linked = linked || in_a;
                    dup = dup || (in_a && in_b);
                }
                const int n_link = __popcll(__ballot(active && a != v && linked));
                const bool judged = active && !has_v;
                const bool valid = n_link == 2 && __ballot(judged && (!ok || dup)) == 0;
                long long term = 0;
                if (judged && ok) term = (long long)rint(fmin(((g * g) / len) * kc, CAP));
                const long long cost = wave_sum(term);
                const long long vlen = (long long)rint(fmin(((dv0 * dv0 + dv1 * dv1) + dv2 * dv2) * kl, CAP));
                if (valid && (tgt < 0 || cost < best_cost || (cost == best_cost && (vlen < best_len || (vlen == best_len && v < tgt))))) {
                    best_cost = cost;
                    best_len = vlen;
                    tgt = v;
                }
            }
            if (tgt >= 0) {
                key = ((u64)code(best_cost) << 32) | mix((unsigned)u);
                if (active) atomicMin(claim + a, key);
                if (lane == 0) atomicMin(claim + u, key);
            }
        }
    }
    if (lane == 0) {
        ckey[u] = key;
        target[u] = tgt;
    }
}

__global__ __launch_bounds__(THREADS) void md_win(const int* __restrict__ cur, const int* __restrict__ degree, const int* __restrict__ start,
                                                  const int* __restrict__ rows, long long n_v, const u64* __restrict__ claim,
                                                  const u64* __restrict__ ckey, u64* __restrict__ wkey, Counters* counters) {
    const long long u = (long long)blockIdx.x * THREADS + threadIdx.x;
    const u64 key = u < n_v ? ckey[u] : NONE;
    const bool cand = key != NONE;
    bool won = cand;
    if (cand) {
        won = claim[u] == key;
        const int d = degree[u], s = start[u];          // d <= MAX_DEGREE: u is a candidate
        for (int q = 0; q < d && won; ++q) {
            const int r = rows[s + q];
            const int f = r / 3, j = r - 3 * f;
            won = claim[cur[3 * (size_t)f + (j + 1) % 3]] == key;
        }
        if (won) wkey[u] = key;                         // NONE otherwise, from the clear
    }
    const u64 mc = __ballot(cand), mw = __ballot(won);
    if ((threadIdx.x & 63) == 0) {
        if (mc) atomicAdd(&counters->candidates, (u64)__popcll(mc));
        if (mw) atomicAdd(&counters->winners, (u64)__popcll(mw));
    }
}

__global__ void md_totals(const Counters* __restrict__ counters, long long* __restrict__ totals) {
    totals[0] = (long long)counters->candidates;
    totals[1] = (long long)counters->winners;
    totals[2] = (long long)counters->faces;
}

// the n_keep-th smallest of the winners' keys (they differ), eight bits at a time from the top, by one workgroup
__global__ __launch_bounds__(SELECT_THREADS) void md_select(const u64* __restrict__ wkey, long long n_v, long long n_keep, Counters* counters) {
    __shared__ unsigned hist[256];
    __shared__ u64 s_prefix;
    __shared__ long long s_left;
    if (threadIdx.x == 0) {
        s_prefix = 0;
        s_left = n_keep;
    }
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (threadIdx.x < 256) hist[threadIdx.x] = 0;
        __syncthreads();
        const u64 prefix = s_prefix;
        for (long long v = threadIdx.x; v < n_v; v += SELECT_THREADS) {
            const u64 k = wkey[v];
            if (k == NONE) continue;
            if (shift == 56 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            long long left = s_left;
            int digit = 0;
            while (digit < 255 && left > (long long)hist[digit]) left -= hist[digit++];
            s_left = left;
            s_prefix = prefix | ((u64)digit << shift);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) counters->threshold = s_prefix;
}

__global__ void md_all(Counters* counters) { counters->threshold = NONE - 1; }

__global__ __launch_bounds__(THREADS) void md_rewrite(int* cur, long long n_f, const u64* __restrict__ wkey, const int* __restrict__ target,
                                                      const Counters* __restrict__ counters) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_f || cur[3 * f] < 0) return;
    const u64 threshold = counters->threshold;
    int x[3];
    bool changed = false;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        x[j] = cur[3 * f + j];
        if (wkey[x[j]] <= threshold) {
            x[j] = target[x[j]];
            changed = true;
        }
    }
    if (!changed) return;
    const bool dead = x[0] == x[1] || x[1] == x[2] || x[0] == x[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) cur[3 * f + j] = dead ? -1 : x[j];
}

// the compaction's rule: every current face (a dead one holds -1 and fails the range test before the rule is asked)
struct Alive {
    __device__ bool operator()(const int[3]) const { return true; }
};

inline bool range_ok(int64_t n_v, int64_t n_f) { return n_v <= INT32_MAX && n_f <= NGP_MESHDECIMATE_MAX_FACES; }

inline bool float_ok(float x) { return x >= -3.402823466e38f && x <= 3.402823466e38f; }       // false for NaN

inline unsigned grid_of(long long n, int per) { return (unsigned)blocks_of(n, per); }

}  // namespace

NGP_API int ngp_meshdecimate_abi_version(void) { return 1; }

NGP_API const char* ngp_meshdecimate_build_arch(void) { return "gfx950"; }

NGP_API size_t ngp_meshdecimate_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    if (n_vertices < 0 || n_faces < 0 || !range_ok(n_vertices, n_faces)) return 0;
    return carve(nullptr, n_vertices, n_faces).total;
}

NGP_API int ngp_meshdecimate_begin(const int32_t* faces, int64_t n_vertices, int64_t n_faces, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (n_vertices < 0 || n_faces < 0) return NGP_EINVAL;
    if (!range_ok(n_vertices, n_faces)) return NGP_ERANGE;
    if (n_faces == 0) return 0;
    if (!faces || !workspace) return NGP_EINVAL;
    const Ws w = carve((char*)workspace, n_vertices, n_faces);
    if (workspace_bytes < w.total) return NGP_EINVAL;
    hipLaunchKernelGGL(md_init, dim3(grid_of(n_faces, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, faces, (long long)n_vertices,
                       (long long)n_faces, w.faces);
    return launched();
}

NGP_API int ngp_meshdecimate_round(const float* vertices, int64_t n_vertices, int64_t n_faces, float cell, float max_error, void* workspace,
                                   size_t workspace_bytes, int64_t* totals, void* stream) {
    if (n_vertices < 0 || n_faces < 0 || !(cell > 0.f && cell <= 3.402823466e38f) || !float_ok(max_error) || !totals) return NGP_EINVAL;
    if (!range_ok(n_vertices, n_faces)) return NGP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    if (n_vertices == 0 || n_faces == 0) return (int)hipMemsetAsync(totals, 0, 3 * sizeof(int64_t), s);
    if (!vertices || !workspace) return NGP_EINVAL;
    const Ws w = carve((char*)workspace, n_vertices, n_faces);
    if (workspace_bytes < w.total) return NGP_EINVAL;
    const long long n_v = n_vertices, n_f = n_faces;
    const double c = (double)cell;
    const double kc = SD / ((c * c) * c), kl = SD / (c * c);
    const double e2 = max_error < 0.f ? -1.0 : (double)max_error * (double)max_error;
    hipError_t e = hipMemsetAsync(w.degree, 0, w.zero_bytes, s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(w.claim, 0xFF, w.none_bytes, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(md_count, dim3(grid_of(n_f, THREADS)), dim3(THREADS), 0, s, (const int*)w.faces, n_f, w.degree, w.counters);
    hipLaunchKernelGGL(md_alloc, dim3(grid_of(n_v, THREADS)), dim3(THREADS), 0, s, (const int*)w.degree, n_v, w.start, w.counters);
    hipLaunchKernelGGL(md_fill, dim3(grid_of(n_f, THREADS)), dim3(THREADS), 0, s, (const int*)w.faces, n_f, (const int*)w.start, w.filled,
                       w.rows);
    hipLaunchKernelGGL(md_eval, dim3(grid_of(n_v, WAVES)), dim3(THREADS), 0, s, vertices, (const int*)w.faces, (const int*)w.degree,
                       (const int*)w.start, (const int*)w.rows, n_v, e2, kc, kl, w.claim, w.ckey, w.target);
    hipLaunchKernelGGL(md_win, dim3(grid_of(n_v, THREADS)), dim3(THREADS), 0, s, (const int*)w.faces, (const int*)w.degree,
                       (const int*)w.start, (const int*)w.rows, n_v, (const u64*)w.claim, (const u64*)w.ckey, w.wkey, w.counters);
    hipLaunchKernelGGL(md_totals, dim3(1), dim3(1), 0, s, (const Counters*)w.counters, (long long*)totals);
    return launched();
}

NGP_API int ngp_meshdecimate_apply(int64_t n_vertices, int64_t n_faces, int64_t n_winners, int64_t n_keep, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    if (n_vertices < 0 || n_faces < 0 || n_keep < 0 || n_keep > n_winners || n_winners > n_vertices) return NGP_EINVAL;
    if (!range_ok(n_vertices, n_faces)) return NGP_ERANGE;
    if (n_keep == 0 || n_faces == 0) return 0;
    if (!workspace) return NGP_EINVAL;
    const Ws w = carve((char*)workspace, n_vertices, n_faces);
    if (workspace_bytes < w.total) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long n_v = n_vertices, n_f = n_faces;
    if (n_keep < n_winners)
        hipLaunchKernelGGL(md_select, dim3(1), dim3(SELECT_THREADS), 0, s, (const u64*)w.wkey, n_v, (long long)n_keep, w.counters);
    else
        hipLaunchKernelGGL(md_all, dim3(1), dim3(1), 0, s, w.counters);
    hipLaunchKernelGGL(md_rewrite, dim3(grid_of(n_f, THREADS)), dim3(THREADS), 0, s, w.faces, n_f, (const u64*)w.wkey, (const int*)w.target,
                       (const Counters*)w.counters);
    return launched();
}

NGP_API int ngp_meshdecimate_count(int64_t n_vertices, int64_t n_faces, void* workspace, size_t workspace_bytes, int64_t* totals,
                                   void* stream) {
    if (n_vertices < 0 || n_faces < 0 || !totals) return NGP_EINVAL;
    if (!range_ok(n_vertices, n_faces)) return NGP_ERANGE;
    if (n_vertices == 0 || n_faces == 0) return (int)hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), (hipStream_t)stream);
    if (!workspace) return NGP_EINVAL;
    const Ws w = carve((char*)workspace, n_vertices, n_faces);
    if (workspace_bytes < w.total) return NGP_EINVAL;
    return compact_count(Alive{}, (const int*)w.faces, n_vertices, n_faces, w.compact, (long long*)totals, (hipStream_t)stream);
}

NGP_API int ngp_meshdecimate_emit(const float* vertices, const float* normals, const float* colors, int64_t n_vertices, int64_t n_faces,
                                  void* workspace, size_t workspace_bytes, int64_t n_out_vertices, int64_t n_out_faces, float* vertices_out,
                                  float* normals_out, float* colors_out, int32_t* faces_out, void* stream) {
    if (n_vertices < 0 || n_faces < 0 || n_out_vertices < 0 || n_out_faces < 0 || n_out_vertices > n_vertices || n_out_faces > n_faces)
        return NGP_EINVAL;
    if (!range_ok(n_vertices, n_faces)) return NGP_ERANGE;
    if (n_out_vertices == 0 && n_out_faces == 0) return 0;
    if (!workspace) return NGP_EINVAL;
    if (n_out_vertices > 0 && (!vertices || !vertices_out || !normals != !normals_out || !colors != !colors_out)) return NGP_EINVAL;
    if (n_out_faces > 0 && !faces_out) return NGP_EINVAL;
    const Ws w = carve((char*)workspace, n_vertices, n_faces);
    if (workspace_bytes < w.total) return NGP_EINVAL;
    return compact_emit(Alive{}, (const int*)w.faces, vertices, normals, colors, n_vertices, n_faces, w.compact, n_out_vertices, n_out_faces,
                        vertices_out, normals_out, colors_out, faces_out, (hipStream_t)stream);
}
