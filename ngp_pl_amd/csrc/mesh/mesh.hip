// libngp_mesh.so: marching cubes over a sampled density volume (C ABI: include/ngp_mesh.h).
//
// Bricks are contiguous ranges of BRICK lattice points in linear order (256 threads x MC_ITERS rounds, lane-contiguous in
// every round), so a brick's vertices and triangles are a contiguous range of the output and a prefix sum over bricks places
// them.  Four launches, all on the caller's stream:
//   mc_count            reads the volume once: per point a flag byte (bit 0 inside, bits 1-3 crossed +x/+y/+z edges), per
//                       brick the packed (triangles << 16 | vertices) count;
//   mc_scan_bricks      one workgroup: exclusive int64 scan of the brick counts, totals to the caller;
//   mc_emit_vertices    scans the flags within the brick, writes each vertex (position, normal; the volume is read only at
//                       crossed edges) and the point's int32 vertex offset;
//   mc_emit_faces       reads the flags and vertex offsets of each cell's 8 corners (the volume is not read again).
// Workspace: 5 B per point + 20 B per brick.  Every ordering is fixed by linear index, so the output is bit-identical from run
// to run.  Compiled with -ffp-contract=off: positions and normals are the plain f32 expressions of the header, as
// tests/mc_reference.py writes them in numpy.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/ngp_mesh.h"

#define NGP_MC_STORAGE static __constant__ const
#include "mc_tables.h"

namespace {

#include "../mesh_host.h"
#include "../mesh_scan.h"
#include "../mesh_mc.h"

constexpr int MC_THREADS = 256;
constexpr int MC_ITERS = 8;
constexpr int BRICK = MC_THREADS * MC_ITERS;
constexpr int MAX_AXIS = 65535;
constexpr long long MAX_POINTS = 1LL << 36;
static_assert(3 * BRICK < (1 << 16) && NGP_MC_MAX_TRIS * BRICK < (1 << 15), "packed brick counts overflow");

struct Dims {
    int nx, ny, nz;
    long long nxny, n;
};

struct Geom {
    float lo[3], h[3];
};

__device__ inline void decode(long long p, const Dims& d, int& i, int& j, int& k) {
    unsigned long long row = (unsigned long long)p / (unsigned)d.nx;
    i = (int)(p - (long long)row * d.nx);
    unsigned long long kk = row / (unsigned)d.ny;
    k = (int)kk;
    j = (int)(row - kk * d.ny);
}

__global__ __launch_bounds__(MC_THREADS) void mc_count(const float* __restrict__ vol, Dims d, float thr,
                                                       uint8_t* __restrict__ flags, int* __restrict__ brick_counts) {
    __shared__ int lds4[MC_THREADS / 64];
    const long long base = (long long)blockIdx.x * BRICK;
    int acc = 0;
    for (int r = 0; r < MC_ITERS; ++r) {
        const long long p = base + r * MC_THREADS + threadIdx.x;
        if (p >= d.n) break;
        int i, j, k;
        decode(p, d, i, j, k);
        const bool hx = i + 1 < d.nx, hy = j + 1 < d.ny, hz = k + 1 < d.nz;
        const int in0 = mc_inside(vol[p], thr);
        const int inx = hx ? mc_inside(vol[p + 1], thr) : in0;
        const int iny = hy ? mc_inside(vol[p + d.nx], thr) : in0;
        const int inz = hz ? mc_inside(vol[p + d.nxny], thr) : in0;
        const int mask = (inx != in0) | (iny != in0) << 1 | (inz != in0) << 2;
        int tris = 0;
        if (hx && hy && hz) {
            const int cube = in0 | inx << 1 | iny << 2 | mc_inside(vol[p + d.nx + 1], thr) << 3 | inz << 4 |
                             mc_inside(vol[p + d.nxny + 1], thr) << 5 | mc_inside(vol[p + d.nxny + d.nx], thr) << 6 |
                             mc_inside(vol[p + d.nxny + d.nx + 1], thr) << 7;
            tris = NGP_MC_TRI_COUNT[cube];
        }
        flags[p] = (uint8_t)(in0 | mask << 1);
        acc += __popc(mask) | tris << 16;
    }
    const int total = block_sum<MC_THREADS>(acc, lds4);    // of the packed counts (fits: static_assert above)
    if (threadIdx.x == 0) brick_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(SCAN_THREADS) void mc_scan_bricks(const int* __restrict__ brick_counts, int nb,
                                                               long long* __restrict__ brick_offsets, long long* __restrict__ totals) {
    // scan_array of ../mesh_scan.h restated for the two packed fields at once, on purpose: two calls of it, one per half-word,
    // read the 64 counts a thread has at 512^3 four times instead of twice and cost marching cubes 0.1 ms there
    __shared__ long long sv[2][SCAN_THREADS], st[2][SCAN_THREADS];
    const int t = threadIdx.x;
    const int per = (nb + SCAN_THREADS - 1) / SCAN_THREADS;
    const int b0 = min(nb, t * per), b1 = min(nb, b0 + per);
    long long v = 0, f = 0;
    for (int b = b0; b < b1; ++b) {
        const int c = brick_counts[b];
        v += c & 0xffff;
        f += c >> 16;
    }
    int cur = 0;
    sv[0][t] = v;
    st[0][t] = f;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {        // inclusive Hillis-Steele over the per-thread sums
        long long a = sv[cur][t], b = st[cur][t];
        if (t >= o) {
            a += sv[cur][t - o];
            b += st[cur][t - o];
        }
        sv[cur ^ 1][t] = a;
        st[cur ^ 1][t] = b;
        cur ^= 1;
        __syncthreads();
    }
    long long ov = sv[cur][t] - v, of = st[cur][t] - f;
    for (int b = b0; b < b1; ++b) {
        const int c = brick_counts[b];
        brick_offsets[2 * b] = ov;
        brick_offsets[2 * b + 1] = of;
        ov += c & 0xffff;
        of += c >> 16;
    }
    if (t == SCAN_THREADS - 1) {
        totals[0] = sv[cur][t];
        totals[1] = st[cur][t];
    }
}

__device__ inline float grad_axis(const float* __restrict__ vol, long long q, int c, int n, long long stride, float h) {
    return mc_grad_axis([=](int s) { return vol[q + s * stride]; }, c, n, h);
}

__device__ inline void gradient(const float* __restrict__ vol, const Dims& d, const Geom& g, long long q, int i, int j, int k,
                                float out[3]) {
    out[0] = grad_axis(vol, q, i, d.nx, 1, g.h[0]);
    out[1] = grad_axis(vol, q, j, d.ny, d.nx, g.h[1]);
    out[2] = grad_axis(vol, q, k, d.nz, d.nxny, g.h[2]);
}

__global__ __launch_bounds__(MC_THREADS) void mc_emit_vertices(const float* __restrict__ vol, Dims d, float thr, Geom g,
                                                               const uint8_t* __restrict__ flags, const long long* __restrict__ brick_offsets,
                                                               int* __restrict__ voff, long long cap, float* __restrict__ verts,
                                                               float* __restrict__ normals) {
    __shared__ int lds4[MC_THREADS / 64];
    const long long base = (long long)blockIdx.x * BRICK;
    long long carry = brick_offsets[2 * blockIdx.x];
    for (int r = 0; r < MC_ITERS; ++r) {
        const long long p = base + r * MC_THREADS + threadIdx.x;
        const bool live = p < d.n;                      // block-uniform loop: every thread takes part in the scan
        const int mask = live ? flags[p] >> 1 : 0;
        int total;
        const long long v0 = carry + block_exscan<MC_THREADS, int>(__popc(mask), total, lds4);
        carry += total;
        if (!live) continue;
        voff[p] = (int)v0;                              // fits: the caller's total is <= INT32_MAX (ngp_mesh_emit)
        if (!mask) continue;
        int idx[3];
        decode(p, d, idx[0], idx[1], idx[2]);
        const float sa = vol[p];
        float ga[3];
        gradient(vol, d, g, p, idx[0], idx[1], idx[2], ga);
        float pa[3];
        for (int a = 0; a < 3; ++a) pa[a] = mc_position(g.lo[a], g.h[a], idx[a]);
        long long vi = v0;
        for (int a = 0; a < 3; ++a) {
            if (!(mask >> a & 1)) continue;
            const long long stride = a == 0 ? 1 : a == 1 ? (long long)d.nx : d.nxny;
            const long long q = p + stride;
            const float sb = vol[q];
            const float t = mc_edge_t(thr, sa, sb);
            int jdx[3] = {idx[0], idx[1], idx[2]};
            jdx[a] += 1;
            float gb[3];
            gradient(vol, d, g, q, jdx[0], jdx[1], jdx[2], gb);
            if (vi < cap) mc_vertex(pa, a, mc_position(g.lo[a], g.h[a], jdx[a]), t, ga, gb, verts + 3 * vi, normals ? normals + 3 * vi : nullptr);
            ++vi;
        }
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_emit_faces(Dims d, const uint8_t* __restrict__ flags, const int* __restrict__ voff,
                                                            const long long* __restrict__ brick_offsets, long long cap,
                                                            int* __restrict__ faces) {
    __shared__ int lds4[MC_THREADS / 64];
    const long long base = (long long)blockIdx.x * BRICK;
    long long carry = brick_offsets[2 * blockIdx.x + 1];
    for (int r = 0; r < MC_ITERS; ++r) {
        const long long p = base + r * MC_THREADS + threadIdx.x;
        int i = 0, j = 0, k = 0;
        if (p < d.n) decode(p, d, i, j, k);
        const bool cell = p < d.n && i + 1 < d.nx && j + 1 < d.ny && k + 1 < d.nz;
        long long off[8];
        int cube = 0;
        if (cell) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                off[c] = p + (c & 1) + ((c >> 1) & 1) * (long long)d.nx + ((c >> 2) & 1) * d.nxny;
                cube |= (flags[off[c]] & 1) << c;
            }
        }
        const int nt = NGP_MC_TRI_COUNT[cube];
        int total;
        const long long f0 = carry + block_exscan<MC_THREADS>(nt, total, lds4);
        carry += total;
        for (int tr = 0; tr < nt; ++tr) {
            if (f0 + tr >= cap) break;
            for (int c = 0; c < 3; ++c) {
                int corner, axis;
                mc_face_corner(cube, tr, c, corner, axis);
                const long long q = off[corner];
                const int before = (flags[q] >> 1) & ((1 << axis) - 1);
                faces[3 * (f0 + tr) + c] = voff[q] + __popc(before);
            }
        }
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_lattice_points(Dims d, Geom g, long long begin, long long count, float* __restrict__ xyz) {
    const long long s = (long long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (s >= count) return;
    int idx[3];
    decode(begin + s, d, idx[0], idx[1], idx[2]);
    for (int a = 0; a < 3; ++a) xyz[3 * s + a] = mc_position(g.lo[a], g.h[a], idx[a]);
}

bool dims_ok(int nx, int ny, int nz, Dims& d) {
    if (nx < 2 || ny < 2 || nz < 2 || nx > MAX_AXIS || ny > MAX_AXIS || nz > MAX_AXIS) return false;
    d.nx = nx;
    d.ny = ny;
    d.nz = nz;
    d.nxny = (long long)nx * ny;
    d.n = d.nxny * nz;
    return d.n <= MAX_POINTS;
}

struct Layout {
    size_t flags, voff, counts, offsets, total;
    long long nb;
};

Layout layout(const Dims& d) {
    Layout l;
    l.nb = (d.n + BRICK - 1) / BRICK;
    l.flags = 0;
    l.voff = align256((size_t)d.n);
    l.counts = l.voff + align256((size_t)d.n * 4);
    l.offsets = l.counts + align256((size_t)l.nb * 4);
    l.total = l.offsets + (size_t)l.nb * 16;
    return l;
}

bool geom_ok(const Dims& d, const float* b6, Geom& g) {
    const int n[3] = {d.nx, d.ny, d.nz};
    for (int a = 0; a < 3; ++a) {
        const float lo = b6[a], hi = b6[3 + a];
        if (!(hi > lo) || !(hi - lo < 3.0e38f)) return false;      // also rejects NaN and infinities
        g.lo[a] = lo;
        g.h[a] = (hi - lo) / (float)(n[a] - 1);
    }
    return true;
}

}  // namespace

NGP_API int ngp_mesh_abi_version(void) { return 1; }

NGP_API const char* ngp_mesh_build_arch(void) { return "gfx950"; }

NGP_API size_t ngp_mesh_workspace_bytes(int nx, int ny, int nz) {
    Dims d;
    if (!dims_ok(nx, ny, nz, d)) return 0;
    return layout(d).total;
}

NGP_API int ngp_mesh_lattice_points(int nx, int ny, int nz, const float* bounds6, int64_t begin, int64_t count, float* xyz, void* stream) {
    Dims d;
    Geom g;
    if (!dims_ok(nx, ny, nz, d) || !bounds6 || begin < 0 || count < 0 || begin + count > d.n) return NGP_EINVAL;
    if (count == 0) return 0;
    if (!xyz || !geom_ok(d, bounds6, g)) return NGP_EINVAL;
    const long long blocks = (count + MC_THREADS - 1) / MC_THREADS;
    hipLaunchKernelGGL(mc_lattice_points, dim3((unsigned)blocks), dim3(MC_THREADS), 0, (hipStream_t)stream, d, g, (long long)begin,
                       (long long)count, xyz);
    return launched();
}

NGP_API int ngp_mesh_count(const float* volume, int nx, int ny, int nz, float threshold, void* workspace, size_t workspace_bytes,
                           int64_t* totals, void* stream) {
    Dims d;
    if (!dims_ok(nx, ny, nz, d) || !volume || !workspace || !totals) return NGP_EINVAL;
    const Layout l = layout(d);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_count, dim3((unsigned)l.nb), dim3(MC_THREADS), 0, s, volume, d, threshold, (uint8_t*)(ws + l.flags),
                       (int*)(ws + l.counts));
    hipLaunchKernelGGL(mc_scan_bricks, dim3(1), dim3(SCAN_THREADS), 0, s, (const int*)(ws + l.counts), (int)l.nb,
                       (long long*)(ws + l.offsets), (long long*)totals);
    return launched();
}

NGP_API int ngp_mesh_emit(const float* volume, int nx, int ny, int nz, float threshold, const float* bounds6, void* workspace,
                          size_t workspace_bytes, int64_t n_vertices, int64_t n_faces, float* vertices, float* normals, int32_t* faces,
                          void* stream) {
    Dims d;
    Geom g;
    if (!dims_ok(nx, ny, nz, d) || !volume || !bounds6 || !workspace || n_vertices < 0 || n_faces < 0) return NGP_EINVAL;
    if ((n_vertices > 0 && !vertices) || (n_faces > 0 && !faces) || !geom_ok(d, bounds6, g)) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    const Layout l = layout(d);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    if (n_vertices == 0 && n_faces == 0) return 0;
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(mc_emit_vertices, dim3((unsigned)l.nb), dim3(MC_THREADS), 0, s, volume, d, threshold, g,
                       (const uint8_t*)(ws + l.flags), (const long long*)(ws + l.offsets), (int*)(ws + l.voff), (long long)n_vertices,
                       vertices, normals);
    hipLaunchKernelGGL(mc_emit_faces, dim3((unsigned)l.nb), dim3(MC_THREADS), 0, s, d, (const uint8_t*)(ws + l.flags),
                       (const int*)(ws + l.voff), (const long long*)(ws + l.offsets), (long long)n_faces, faces);
    return launched();
}
