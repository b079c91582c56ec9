// libngp_meshnormal.so: the normals of a detail mesh carried onto query points through the nearest face that faces the same way,
// and the shading of a frame by a rendered normal map (C ABI, the exact rule and why the grid never changes a bit of it:
// ngp_meshnormal.h beside this file).  Compiled with -ffp-contract=off: every f32 expression below is the header's, operation by
// operation.
//
//   transfer   one query per lane, workgroups of 256.  Texels come in row-major atlas order, so the 64 lanes of a wave are
//              neighbours on one or two faces of the simplified mesh and walk the same cell lists of the detail mesh's grid: the
//              list, index and vertex loads of a wave hit the same lines.  The best key lives in one 64-bit register pair; the
//              barycentric pair is recomputed for the winner once the walk is over, so nothing per candidate is kept and there is
//              no per-thread array.  An invalid texel leaves before it loads anything else.
//   shade      one pixel per lane.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ngp_meshnormal.h"

#define NGP_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int THREADS = 256;
constexpr float SLACK_FACTOR = (float)NGP_MESHNORMAL_SLACK_ULPS * 0x1p-23f;
constexpr int MAX_WH = 16384;

struct V3 {
    float x, y, z;
};
__device__ inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline V3 load3(const float* __restrict__ p, long long i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ inline bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
__device__ inline float absmax3(V3 a) { return fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fabsf(a.z)); }

// the three vertices of a usable face; false otherwise
__device__ inline bool load_face(const float* __restrict__ v, const int32_t* __restrict__ f, int n_v, long long face, V3& a, V3& b, V3& c) {
    const int ia = f[3 * face], ib = f[3 * face + 1], ic = f[3 * face + 2];
    if ((unsigned)ia >= (unsigned)n_v || (unsigned)ib >= (unsigned)n_v || (unsigned)ic >= (unsigned)n_v) return false;
    a = load3(v, ia);
    b = load3(v, ib);
    c = load3(v, ic);
    return finite3(a) && finite3(b) && finite3(c);
}

// rule 1: the face faces the way m does
__device__ inline bool faces_along(V3 a, V3 b, V3 c, V3 m) {
    const V3 ab = sub(b, a), ac = sub(c, a);
    const V3 g = {ab.y * ac.z - ab.z * ac.y, ab.z * ac.x - ab.x * ac.z, ab.x * ac.y - ab.y * ac.x};
    return dot(g, m) > 0.0f;
}

// rule 2: the closest point of (a, b, c) to p and the barycentric pair of the deciding case
__device__ inline V3 closest_point(V3 p, V3 a, V3 b, V3 c, float& bv, float& bw) {
    const V3 ab = sub(b, a), ac = sub(c, a), ap = sub(p, a);
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    bv = 0.0f, bw = 0.0f;
    if (d1 <= 0.0f && d2 <= 0.0f) return a;
    const V3 bp = sub(p, b);
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.0f && d4 <= d3) {
        bv = 1.0f;
        return b;
    }
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float v = d1 / (d1 - d3);
        bv = v;
        return {a.x + v * ab.x, a.y + v * ab.y, a.z + v * ab.z};
    }
    const V3 cp = sub(p, c);
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0f && d5 <= d6) {
        bw = 1.0f;
        return c;
    }
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float w = d2 / (d2 - d6);
        bw = w;
        return {a.x + w * ac.x, a.y + w * ac.y, a.z + w * ac.z};
    }
    const float va = d3 * d6 - d5 * d4;
    const float s43 = d4 - d3, s56 = d5 - d6;
    if (va <= 0.0f && s43 >= 0.0f && s56 >= 0.0f) {
        const float w = s43 / (s43 + s56);
        const V3 bc = sub(c, b);
        bv = 1.0f - w, bw = w;
        return {b.x + w * bc.x, b.y + w * bc.y, b.z + w * bc.z};
    }
    const float denom = 1.0f / ((va + vb) + vc);
    float v = vb * denom, w = vc * denom;
    if (!(v >= 0.0f)) v = 0.0f;
    if (v > 1.0f) v = 1.0f;
    if (!(w >= 0.0f)) w = 0.0f;
    const float rest = 1.0f - v;
    if (w > rest) w = rest;
    bv = v, bw = w;
    return {(a.x + v * ab.x) + w * ac.x, (a.y + v * ab.y) + w * ac.y, (a.z + v * ab.z) + w * ac.z};
}

__device__ inline float squared_distance(V3 p, V3 q) {
    const V3 e = sub(p, q);
    return (e.x * e.x + e.y * e.y) + e.z * e.z;
}

// THE GRID: the clamped cell of a coordinate
__device__ inline int cell_of(float t, float o, float cell, int n) {
    const float g = floorf((t - o) / cell);
    if (!(g >= 0.0f)) return 0;
    if (g >= (float)n) return n - 1;
    return (int)g;
}

struct Grid {
    float ox, oy, oz, cell, m_grid;
    int nx, ny, nz;
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
    unsigned long long best = ~0ull;                        // bits(d2) << 32 | face
    int shells = 0, evaluated = 0;
    const float sq = SLACK_FACTOR * fmaxf(g.m_grid, absmax3(p));
    const int cx = cell_of(p.x, g.ox, g.cell, g.nx), cy = cell_of(p.y, g.oy, g.cell, g.ny), cz = cell_of(p.z, g.oz, g.cell, g.nz);
    for (int r = 0;; ++r) {
        ++shells;
        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.nz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.ny - 1);
        for (int z = z0; z <= z1; ++z) {
            const bool zface = z == cz - r || z == cz + r;
            for (int y = y0; y <= y1; ++y) {
                // a row of the shell: all of [cx - r, cx + r] on a z or y face of the cube, else its two ends
                const bool full = zface || y == cy - r || y == cy + r;
                const int step = full || r == 0 ? 1 : 2 * r;
                for (int x = cx - r; x <= cx + r; x += step) {
                    if (x < 0 || x >= g.nx) continue;
                    const long long cell = ((long long)z * g.ny + y) * g.nx + x;
                    const uint32_t e0 = start[cell], e1 = min(start[cell + 1], (uint32_t)n_entries);
                    for (uint32_t e = e0; e < e1; ++e) {
                        const int face = entries[e];
                        if ((unsigned)face >= (unsigned)n_f) continue;
                        V3 a, b, c;
                        if (!load_face(v, f, n_v, face, a, b, c)) continue;
                        if (oriented && !faces_along(a, b, c, m)) continue;
                        float bv, bw;
                        const float d2 = squared_distance(p, closest_point(p, a, b, c, bv, bw));
                        ++evaluated;
                        if (!(d2 <= 3.402823466e38f)) continue;                 // not finite: contributes nothing
                        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)face;
                        best = key < best ? key : best;
                    }
                }
            }
        }
        const float rc = (float)r * g.cell;
        const float best_d2 = __uint_as_float((uint32_t)(best >> 32));          // NaN bits while nothing was found: the test is false
        if (sqrtf(best_d2) + sq <= rc) break;
        if (rc - sq > max_dist) break;
        const int q = r + 1;                                // the next shell lies wholly outside the grid
        if (cx - q < 0 && cx + q >= g.nx && cy - q < 0 && cy + q >= g.ny && cz - q < 0 && cz + q >= g.nz) break;
    }
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
    if (debug) debug[2 * i] = shells, debug[2 * i + 1] = evaluated;
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

inline int launched() { return (int)hipGetLastError(); }

inline long long scan_blocks(long long n) { return (n + NGP_MESHNORMAL_SCAN_BLOCK - 1) / NGP_MESHNORMAL_SCAN_BLOCK; }

inline bool axes_ok(int nx, int ny, int nz) {
    const int m = NGP_MESHNORMAL_MAX_AXIS;
    return nx >= 1 && ny >= 1 && nz >= 1 && nx <= m && ny <= m && nz <= m && (long long)nx * ny * nz <= NGP_MESHNORMAL_MAX_CELLS;
}

// M_grid of the header, or a negative value for a grid that is refused
inline float grid_magnitude(const float* origin, float cell, int nx, int ny, int nz) {
    if (!origin || !axes_ok(nx, ny, nz) || !(cell > 0.0f) || !isfinite(cell)) return -1.0f;
    const int n[3] = {nx, ny, nz};
    float m = 0.0f;
    for (int k = 0; k < 3; ++k) {
        if (!isfinite(origin[k])) return -1.0f;
        const float far = origin[k] + (float)n[k] * cell;
        if (!isfinite(far)) return -1.0f;
        m = fmaxf(m, fmaxf(fabsf(origin[k]), fabsf(far)));
    }
    return m;
}

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
    const float m = grid_magnitude(origin, cell, nx, ny, nz);
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
