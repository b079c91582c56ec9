// libngp_meshquadric.so: quadric placement of the vertices of a vertex clustering (C ABI and the exact rule:
// include/ngp_meshquadric.h).  Compiled with -ffp-contract=off: every f32 and f64 expression below is the header's, operation by
// operation.
//
// ngp_meshquadric_accumulate, on the caller's stream:
//   clear            the 14 int64 sums of every vertex to 0;
//   mq_members       one thread per vertex: n and P of the vertex go to its label's sums;
//   mq_corners       one thread per corner (3 per face): the corner's plane, weighted by the face's area in cells, goes to the ten
//                    sums A, B, Wsum of the label of the corner's vertex.
//   Both bin vertices with the cell_of of ../mesh_cells.h, the one the clustering of ../meshsimplify/meshsimplify.hip used, and
//   group the lanes of a wave by destination with add_by_label of ../mesh_labels.h, as its cs_sums does: a group of FOLD_MIN lanes
//   or more is summed across the wave and added by one lane (the corners of neighbouring faces land on one cluster, which would
//   otherwise serialise up to 64 adds per instruction on one address), a smaller group adds lane by lane.
// ngp_meshquadric_sums:
//   mq_export        the sums of every leader, zeros elsewhere.
// ngp_meshquadric_place:
//   mq_place         one thread per vertex, non-leaders leave: the regularised 3x3 solve in f64, the position, the state; the
//                    three state counts by one add per wave and state.
// Integer atomics only: every output is bit-identical run to run and for any launch shape.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/ngp_meshquadric.h"

namespace {

#include "../mesh_host.h"
#include "../mesh_cells.h"
#include "../mesh_labels.h"

constexpr int THREADS = 256;
constexpr double SD = 16777216.0;                       // the header's S
constexpr double W_MAX = 16.0;
constexpr double EPS = 0.0009765625;                    // 2^-10
constexpr int SUMS = NGP_MESHQUADRIC_SUMS;              // per label: n, P[3], A[6], B[3], Wsum
constexpr int CORNER_SUMS = 10;                         // A[6], B[3], Wsum: sums 4..13

typedef unsigned long long u64;

__global__ __launch_bounds__(THREADS) void mq_members(const float* __restrict__ vertices, const int* __restrict__ label, long long n_v,
                                                      const float* __restrict__ origin, float cell, u64* sums) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    int l = -1;
    long long val[4] = {};
    if (v < n_v) {
        l = label[v];
        if ((unsigned)l >= (unsigned)n_v) l = -1;
    }
    if (l >= 0) {
        const Grid g = load_grid(origin, cell);
        int c[3];
        if (cell_of(g, vertices + 3 * v, c, val + 1))
            val[0] = 1;
        else
            l = -1;
    }
    add_by_label<4>(l, val, sums, SUMS, 0);
}

__global__ __launch_bounds__(THREADS) void mq_corners(const float* __restrict__ vertices, const int* __restrict__ faces,
                                                      const int* __restrict__ label, long long n_v, long long n_corners,
                                                      const float* __restrict__ origin, float cell, u64* sums) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    int l = -1;
    long long val[CORNER_SUMS] = {};
    if (t < n_corners) {
        const long long f = t / 3;
        const int j = (int)(t - 3 * f);
        const int a = faces[3 * f + j], b = faces[3 * f + (j + 1) % 3], c = faces[3 * f + (j + 2) % 3];
        const unsigned n = (unsigned)n_v;
        if ((unsigned)a < n && (unsigned)b < n && (unsigned)c < n) {
            l = label[a];
            if ((unsigned)l >= n) l = -1;
        }
        if (l >= 0) {
            const Grid g = load_grid(origin, cell);
            const float* xa = vertices + 3 * (size_t)a;
            int ca[3];
            long long q[3];
            bool ok = cell_of(g, xa, ca, q);
            const float* xb = vertices + 3 * (size_t)b;
            const float* xc = vertices + 3 * (size_t)c;
            double e1[3], e2[3], y[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                e1[k] = (double)xb[k] - (double)xa[k];
                e2[k] = (double)xc[k] - (double)xa[k];
                y[k] = (double)q[k] / QD - 0.5;
            }
            double nrm[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            const double len = sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]);
            ok = ok && len > 0.0 && len < __longlong_as_double(0x7FF0000000000000ll);         // false for NaN
            if (ok) {
#pragma unroll
                for (int k = 0; k < 3; ++k) nrm[k] = nrm[k] / len;
                const double w = fmin((0.5 * len) / ((double)g.cell * (double)g.cell), W_MAX);
                const double d = (nrm[0] * y[0] + nrm[1] * y[1]) + nrm[2] * y[2];
                int s = 0;
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int k = i; k < 3; ++k) val[s++] = (long long)rint(((w * nrm[i]) * nrm[k]) * SD);
#pragma unroll
                for (int i = 0; i < 3; ++i) val[6 + i] = (long long)rint(((w * d) * nrm[i]) * SD);
                val[9] = (long long)rint(w * SD);
            } else {
                l = -1;
            }
        }
    }
    add_by_label<CORNER_SUMS>(l, val, sums, SUMS, 4);
}

__global__ __launch_bounds__(THREADS) void mq_export(const int* __restrict__ label, long long n_v, const long long* __restrict__ sums,
                                                     long long* __restrict__ out) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_v * SUMS) return;
    const long long v = i / SUMS;
    out[i] = label[v] == (int)v ? sums[i] : 0;
}

__global__ __launch_bounds__(THREADS) void mq_place(const float* __restrict__ vertices, const int* __restrict__ label, long long n_v,
                                                    const float* __restrict__ origin, float cell, const long long* __restrict__ sums,
                                                    float* __restrict__ positions, uint8_t* __restrict__ state, u64* totals) {
    const long long v = (long long)blockIdx.x * THREADS + threadIdx.x;
    int st = NGP_MESHQUADRIC_NOT_LEADER;
    if (v < n_v && label[v] == (int)v) {
        const Grid g = load_grid(origin, cell);
        int c[3];
        long long q[3];
        if (cell_of(g, vertices + 3 * v, c, q)) {
            const long long* s = sums + (size_t)SUMS * v;
            const double n = (double)s[0];
            double mean[3], y[3] = {};                  // mean: P / n / Q, the simplifier's; y: the quadric's, centred on the cell
#pragma unroll
            for (int k = 0; k < 3; ++k) mean[k] = ((double)s[1 + k] / n) / QD;
            st = NGP_MESHQUADRIC_MEAN_NO_FACES;
            if (s[13] != 0) {
                st = NGP_MESHQUADRIC_MEAN_OUTSIDE;
                const double r = EPS * (double)s[13];
                const double M00 = (double)s[4] + r, M01 = (double)s[5], M02 = (double)s[6];
                const double M11 = (double)s[7] + r, M12 = (double)s[8], M22 = (double)s[9] + r;
                const double g0 = (double)s[10] + r * (mean[0] - 0.5);
                const double g1 = (double)s[11] + r * (mean[1] - 0.5);
                const double g2 = (double)s[12] + r * (mean[2] - 0.5);
                const double d0 = M00;
                const double l10 = M01 / d0, l20 = M02 / d0;
                const double d1 = M11 - l10 * M01;
                const double t = M12 - l20 * M01;
                const double l21 = t / d1;
                const double d2 = (M22 - l20 * M02) - l21 * t;
                const double z0 = g0;
                const double z1 = g1 - l10 * z0;
                const double z2 = (g2 - l20 * z0) - l21 * z1;
                y[2] = z2 / d2;
                y[1] = z1 / d1 - l21 * y[2];
                y[0] = (z0 / d0 - l10 * y[1]) - l20 * y[2];
                // |y| <= 1 is false for NaN and Inf
                if (d0 > 0.0 && d1 > 0.0 && d2 > 0.0 && fabs(y[0]) <= 1.0 && fabs(y[1]) <= 1.0 && fabs(y[2]) <= 1.0)
                    st = NGP_MESHQUADRIC_QUADRIC;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double in_cell = st == NGP_MESHQUADRIC_QUADRIC ? y[k] + 0.5 : mean[k];
                positions[3 * v + k] = (float)((double)g.o[k] + ((double)c[k] + in_cell) * (double)g.cell);
            }
        }
    }
    if (v < n_v) state[v] = (uint8_t)st;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 1; k <= 3; ++k) {
        const u64 m = __ballot(st == k);
        if (lane == 0 && m) atomicAdd(totals + (k - 1), (u64)__popcll(m));
    }
}

inline size_t ws_bytes(long long n_v) {
    const size_t b = align256((size_t)n_v * SUMS * 8);
    return b ? b : 256;
}

}  // namespace

NGP_API int ngp_meshquadric_abi_version(void) { return 1; }

NGP_API const char* ngp_meshquadric_build_arch(void) { return "gfx950"; }

NGP_API size_t ngp_meshquadric_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    if (n_vertices < 0 || n_faces < 0 || n_vertices > INT32_MAX || n_faces > INT32_MAX) return 0;
    return ws_bytes(n_vertices);
}

NGP_API int ngp_meshquadric_accumulate(const float* vertices, const int32_t* faces, const int32_t* vertex_label, int64_t n_vertices,
                                       int64_t n_faces, const float* origin, float cell, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    if (n_vertices < 0 || n_faces < 0 || !cell_ok(cell)) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (n_vertices == 0) return 0;
    if (!vertices || !vertex_label || !origin || !workspace || (n_faces > 0 && !faces)) return NGP_EINVAL;
    if (workspace_bytes < ws_bytes(n_vertices)) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long n_v = n_vertices, n_corners = 3 * (long long)n_faces;                     // below 2^33: the grid fits 32 bits
    const hipError_t e = hipMemsetAsync(workspace, 0, (size_t)n_v * SUMS * 8, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mq_members, dim3((unsigned)blocks_of(n_v, THREADS)), dim3(THREADS), 0, s, vertices, vertex_label, n_v, origin, cell,
                       (u64*)workspace);
    if (n_corners)
        hipLaunchKernelGGL(mq_corners, dim3((unsigned)blocks_of(n_corners, THREADS)), dim3(THREADS), 0, s, vertices, faces, vertex_label, n_v,
                           n_corners, origin, cell, (u64*)workspace);
    return launched();
}

NGP_API int ngp_meshquadric_sums(const int32_t* vertex_label, int64_t n_vertices, const void* workspace, size_t workspace_bytes,
                                 int64_t* sums_out, void* stream) {
    if (n_vertices < 0) return NGP_EINVAL;
    if (n_vertices > INT32_MAX) return NGP_ERANGE;
    if (n_vertices == 0) return 0;
    if (!vertex_label || !workspace || !sums_out) return NGP_EINVAL;
    if (workspace_bytes < ws_bytes(n_vertices)) return NGP_EINVAL;
    const long long n_v = n_vertices;
    hipLaunchKernelGGL(mq_export, dim3((unsigned)blocks_of(n_v * SUMS, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, vertex_label, n_v,
                       (const long long*)workspace, (long long*)sums_out);
    return launched();
}

NGP_API int ngp_meshquadric_place(const float* vertices, const int32_t* vertex_label, int64_t n_vertices, const float* origin, float cell,
                                  const void* workspace, size_t workspace_bytes, float* positions, uint8_t* state, int64_t* totals,
                                  void* stream) {
    if (n_vertices < 0 || !cell_ok(cell)) return NGP_EINVAL;
    if (n_vertices > INT32_MAX) return NGP_ERANGE;
    if (n_vertices == 0) return 0;
    if (!vertices || !vertex_label || !origin || !workspace || !positions || !state || !totals) return NGP_EINVAL;
    if (workspace_bytes < ws_bytes(n_vertices)) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long n_v = n_vertices;
    const hipError_t e = hipMemsetAsync(totals, 0, 3 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(mq_place, dim3((unsigned)blocks_of(n_v, THREADS)), dim3(THREADS), 0, s, vertices, vertex_label, n_v, origin, cell,
                       (const long long*)workspace, positions, state, (u64*)totals);
    return launched();
}
