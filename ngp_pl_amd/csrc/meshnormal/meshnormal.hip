// libngp_meshnormal.so: the normals of a detail mesh carried onto query points through the nearest face that faces the same way,
// and the shading of a frame by a rendered normal map (C ABI, the exact rule and why the grid never changes a bit of it:
// ngp_meshnormal.h beside this file).  Compiled with -ffp-contract=off: every f32 expression below is the header's, operation by
// operation.
//
//   transfer   one query per lane, workgroups of 256.  Texels come in row-major atlas order, so the 64 lanes of a wave are
//              neighbours on one or two faces of the simplified mesh and walk the same cell lists of the detail mesh's grid: the
//              list, index and vertex loads of a wave hit the same lines.  The walk is nearest_face of ../mesh_nearest.h, the one
//              libngp_meshdist.so's query runs, with the filter Oriented; the barycentric pair is recomputed for the winner once
//              the walk is over, so nothing per candidate is kept.  An invalid texel leaves before it loads anything else.
//   shade      one pixel per lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ngp_meshnormal.h"

namespace {

#include "../mesh_host.h"

constexpr int THREADS = 256;
constexpr float SLACK_FACTOR = (float)NGP_MESHNORMAL_SLACK_ULPS * 0x1p-23f;
constexpr int MAX_WH = 16384;

#include "../mesh_nearest.h"

// rule 1: the face faces the way m does
__device__ inline bool faces_along(V3 a, V3 b, V3 c, V3 m) {
    const V3 ab = sub(b, a), ac = sub(c, a);
    const V3 g = {ab.y * ac.z - ab.z * ac.y, ab.z * ac.x - ab.x * ac.z, ab.x * ac.y - ab.y * ac.x};
    return dot(g, m) > 0.0f;
}

// the walk's filter: under `oriented` only the faces that face the way the query's normal m does
struct Oriented {
    V3 m;
    int oriented;
    __device__ bool operator()(V3 a, V3 b, V3 c) const { return !oriented || faces_along(a, b, c, m); }
};

__global__ __launch_bounds__(THREADS) void transfer(const float* __restrict__ points, const float* __restrict__ qnormals,
                                                    const uint8_t* __restrict__ valid, int n, const float* __restrict__ v,
                                                    const int32_t* __restrict__ f, const float* __restrict__ vn, int n_v, int n_f, Grid g,
                                                    float max_dist, float max_d2, int oriented, const uint32_t* __restrict__ start,
                                                    const int32_t* __restrict__ entries, int n_entries, float* __restrict__ out_n,
                                                    float* __restrict__ out_d2, int32_t* __restrict__ out_face, float* __restrict__ bary,
                                                    int32_t* __restrict__ debug) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const float inf = __uint_as_float(0x7F800000u);
    const bool live = valid[i] != 0;
    V3 p = {0.0f, 0.0f, 0.0f};
    if (live) p = load3(points, i);
    if (!live || !finite3(p)) {                             // rule 4, last paragraph
        out_n[3 * i] = 0.0f, out_n[3 * i + 1] = 0.0f, out_n[3 * i + 2] = 0.0f;
        out_d2[i] = inf;
        out_face[i] = -1;
        if (bary) bary[2 * i] = 0.0f, bary[2 * i + 1] = 0.0f;
        if (debug) debug[2 * i] = 0, debug[2 * i + 1] = 0;
        return;
    }
    const V3 m = load3(qnormals, i);
    uint32_t shells = 0, evaluated = 0;
    const unsigned long long best =                         // bits(d2) << 32 | face
        nearest_face(p, Oriented{m, oriented}, v, f, n_v, n_f, g, SLACK_FACTOR, max_dist, start, entries, n_entries, &shells, &evaluated);
    float d2 = __uint_as_float((uint32_t)(best >> 32));
    int face = (int)(uint32_t)best;
    float bv = 0.0f, bw = 0.0f;
    V3 nrm = {0.0f, 0.0f, 0.0f};
    bool have = false;
    if (best == ~0ull || d2 > max_d2) {
        d2 = inf;
        face = -1;
    } else {                                                // rule 4: the winner's (v, w) by rule 2 again, then its corners' normals
        V3 a, b, c;
        load_face(v, f, n_v, face, a, b, c);
        closest_point(p, a, b, c, bv, bw);
        const V3 na = load3(vn, f[3 * face]), nb = load3(vn, f[3 * face + 1]), nc = load3(vn, f[3 * face + 2]);
        const float bu = (1.0f - bv) - bw;
        const V3 N = {(bu * na.x + bv * nb.x) + bw * nc.x, (bu * na.y + bv * nb.y) + bw * nc.y, (bu * na.z + bv * nb.z) + bw * nc.z};
        const float L = sqrtf(dot(N, N));
        if (L > 0.0f && L <= 3.402823466e38f) {
            nrm = {N.x / L, N.y / L, N.z / L};
            have = true;
        }
    }
    if (!have) {                                            // the fallback: the query's own normal, or +z
        const float Lm = sqrtf(dot(m, m));
        if (Lm > 0.0f && Lm <= 3.402823466e38f) nrm = {m.x / Lm, m.y / Lm, m.z / Lm};
        else nrm = {0.0f, 0.0f, 1.0f};
    }
    out_n[3 * i] = nrm.x, out_n[3 * i + 1] = nrm.y, out_n[3 * i + 2] = nrm.z;
    out_d2[i] = d2;
    out_face[i] = face;
    if (bary) bary[2 * i] = bv, bary[2 * i + 1] = bw;
    if (debug) debug[2 * i] = (int32_t)shells, debug[2 * i + 1] = (int32_t)evaluated;
}

__global__ __launch_bounds__(THREADS) void shade(const float* __restrict__ albedo, const float* __restrict__ samples,
                                                 const int32_t* __restrict__ ids, const float* __restrict__ lights, int n_pixels,
                                                 int per_cam, float ambient, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n_pixels) return;
    const V3 al = load3(albedo, i);
    float k = 1.0f;
    if (ids[i] >= 0) {
        const V3 s = load3(samples, i);
        const V3 t = {2.0f * s.x - 1.0f, 2.0f * s.y - 1.0f, 2.0f * s.z - 1.0f};
        const float L = sqrtf(dot(t, t));
        if (L > 0.0f && L <= 3.402823466e38f) {
            const V3 l = load3(lights, i / per_cam);
            const V3 u = {t.x / L, t.y / L, t.z / L};
            const float d = dot(u, l);
            k = ambient + (1.0f - ambient) * (d > 0.0f ? d : 0.0f);
        }
        out[3 * i] = al.x * k, out[3 * i + 1] = al.y * k, out[3 * i + 2] = al.z * k;
        return;
    }
    out[3 * i] = al.x, out[3 * i + 1] = al.y, out[3 * i + 2] = al.z;
}

// ---- host side

inline long long scan_blocks(long long n) { return (n + NGP_MESHNORMAL_SCAN_BLOCK - 1) / NGP_MESHNORMAL_SCAN_BLOCK; }

}  // namespace

NGP_API int ngp_meshnormal_abi_version(void) { return 1; }

NGP_API const char* ngp_meshnormal_build_arch(void) { return "gfx950"; }

NGP_API int ngp_meshnormal_transfer(const float* points, const float* query_normals, const uint8_t* valid, int64_t n, const float* vertices,
                                    const int32_t* faces, const float* vertex_normals, int64_t n_vertices, int64_t n_faces,
                                    const float* origin, float cell, int nx, int ny, int nz, const void* workspace, size_t workspace_bytes,
                                    const int32_t* entries, int64_t n_entries, float max_dist, int oriented, float* normals_out, float* d2,
                                    int32_t* face, float* bary, int32_t* debug, void* stream) {
    if (n < 0 || n_vertices < 0 || n_faces < 0 || n_entries < 0 || !origin || !workspace) return NGP_EINVAL;
    if ((!vertices && n_vertices > 0) || (!vertex_normals && n_vertices > 0) || (!faces && n_faces > 0)) return NGP_EINVAL;
    if (n_entries > 0 && !entries) return NGP_EINVAL;
    if (n > 0 && (!points || !query_normals || !valid || !normals_out || !d2 || !face)) return NGP_EINVAL;
    const float m = grid_magnitude(origin, cell, nx, ny, nz, NGP_MESHNORMAL_MAX_AXIS, NGP_MESHNORMAL_MAX_CELLS);
    if (m < 0.0f) return NGP_EINVAL;
    if (cell < (float)NGP_MESHNORMAL_MIN_CELL_SLACKS * (SLACK_FACTOR * m)) return NGP_EINVAL;
    if (!(max_dist >= 0.0f) || !isfinite(max_dist) || max_dist > (float)NGP_MESHNORMAL_MAX_SHELLS * cell) return NGP_EINVAL;   // THE CAP
    if (n > INT32_MAX || n_vertices > INT32_MAX || n_faces > INT32_MAX || n_entries > INT32_MAX) return NGP_ERANGE;
    const long long cells = (long long)nx * ny * nz;
    const size_t need = 8 * (size_t)scan_blocks(cells) + 4 * (size_t)(cells + 1) + 4 * (size_t)cells;
    if (workspace_bytes < need || ((uintptr_t)workspace & 7) != 0) return NGP_EINVAL;
    if (n == 0) return 0;
    const Grid g = {origin[0], origin[1], origin[2], cell, m, nx, ny, nz};
    const uint32_t* start = (const uint32_t*)((const long long*)workspace + scan_blocks(cells));
    hipLaunchKernelGGL(transfer, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, points, query_normals,
                       valid, (int)n, vertices, faces, vertex_normals, (int)n_vertices, (int)n_faces, g, max_dist, max_dist * max_dist,
                       oriented != 0 ? 1 : 0, start, entries, (int)n_entries, normals_out, d2, face, bary, debug);
    return launched();
}

NGP_API int ngp_meshnormal_shade(const float* albedo, const float* samples, const int32_t* ids, const float* lights, int64_t n_cams, int H,
                                 int W, float ambient, float* out, void* stream) {
    if (n_cams < 0 || W < 1 || H < 1 || W > MAX_WH || H > MAX_WH || !(ambient >= 0.0f && ambient <= 1.0f)) return NGP_EINVAL;
    if (n_cams > 0 && (!albedo || !samples || !ids || !lights || !out)) return NGP_EINVAL;
    if (n_cams > INT32_MAX / ((int64_t)W * H)) return NGP_ERANGE;
    if (n_cams == 0) return 0;
    const int per_cam = W * H;
    const int n_pixels = (int)(n_cams * per_cam);
    hipLaunchKernelGGL(shade, dim3((unsigned)((n_pixels + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, albedo, samples,
                       ids, lights, n_pixels, per_cam, ambient, out);
    return launched();
}
