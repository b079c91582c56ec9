// libngp_meshcull.so: depth-buffer visibility of an indexed triangle mesh against pinhole cameras, and the sub-mesh of the faces
// some camera sees (C ABI and the exact rule: include/ngp_meshcull.h).  Compiled with -ffp-contract=off: every f32 expression
// below is the header's, operation by operation.
//
// Views, per chunk of as many cameras as the caller's depth workspace holds, on the caller's stream:
//   clear            the chunk's buffers to the bits of +inf (hipMemsetD32Async);
//   cull_raster      one work item per (face, camera): a thread holds its face's three vertices in registers and walks the
//                    cameras of the launch (at most CAM_TILE, their R^T and -R^T t in LDS), re-projecting the vertices for each.
//                    A clipped pixel box of at most SMALL_BOX pixels is walked by the face's own lane; larger boxes are collected
//                    with a ballot and walked by the whole wave, one box after the other, the lanes as an 8 x 8 pixel tile that
//                    strides the box.  Both walkers run the same per-pixel function and the buffer takes a minimum, so which of
//                    them visits a pixel changes the time only.  atomicMin on the depth's bits, skipped when an L2 read of the
//                    pixel already holds a smaller or equal depth (the buffer only ever falls, so a skipped write is never missed);
//   cull_test        one thread per vertex walks the same cameras and adds the views it has: a plain per-vertex sum, no atomic.
// Compaction is the shared one of ../mesh_compact.h with the rule ViewsKeep (a face is kept iff a vertex of it has min_views views).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/ngp_meshcull.h"

#define NGP_API extern "C" __attribute__((visibility("default")))

namespace {

#include "../mesh_compact.h"

constexpr int CAM_TILE = 128;                           // cameras per launch: 12 floats each in LDS
constexpr int SMALL_BOX = 64;                           // pixels a lane walks on its own
constexpr int MAX_WH = 16384;
constexpr unsigned INF_BITS = 0x7F800000u;

// per camera of the launch: the 9 entries of R^T, then -R^T t (the header's m and s)
__device__ inline void load_cameras(const float* __restrict__ poses, long long cam0, int nc, float* s_cam) {
    for (int i = threadIdx.x; i < nc; i += blockDim.x) {
        const float* P = poses + 12 * (size_t)(cam0 + i);   // row-major 3 x 4: [R | t]
        float* o = s_cam + 12 * i;
        const float t0 = P[3], t1 = P[7], t2 = P[11];
#pragma unroll
        for (int r = 0; r < 3; ++r) {                   // row r of R^T = column r of R
            const float a = P[r], b = P[4 + r], cc = P[8 + r];
            o[3 * r] = a;
            o[3 * r + 1] = b;
            o[3 * r + 2] = cc;
            o[9 + r] = -(a * t0 + b * t1 + cc * t2);
        }
    }
    __syncthreads();
}

struct Intrinsics {
    float k[9];
};

__device__ inline Intrinsics load_intrinsics(const float* __restrict__ K) {
    Intrinsics in;
#pragma unroll
    for (int i = 0; i < 9; ++i) in.k[i] = K[i];
    return in;
}

__device__ inline void project(const float* o, const Intrinsics& in, float x, float y, float z, float& u, float& v, float& d) {
    const float px = o[0] * x + o[1] * y + o[2] * z + o[9];
    const float py = o[3] * x + o[4] * y + o[5] * z + o[10];
    const float pz = o[6] * x + o[7] * y + o[8] * z + o[11];
    const float ud = in.k[0] * px + in.k[1] * py + in.k[2] * pz, vd = in.k[3] * px + in.k[4] * py + in.k[5] * pz;
    d = in.k[6] * px + in.k[7] * py + in.k[8] * pz;
    u = ud / d;
    v = vd / d;
}

// a face on one camera's screen: the points A, B, C, 1 / d of each, the signed area and the clipped pixel box
struct Tri {
    float ax, ay, bx, by, cx, cy, qa, qb, qc, area;
    int i0, i1, j0, j1;
};

__device__ inline float edge(float ax, float ay, float bx, float by, float px, float py) { return (bx - ax) * (py - ay) - (by - ay) * (px - ax); }

// pixel (i, j) of the camera whose buffer is zb: inside test on the centre, perspective-correct depth, minimum
__device__ inline void shade(const Tri& t, int i, int j, unsigned* zb, int W) {
    const float px = (float)i + 0.5f, py = (float)j + 0.5f;
    const float wa = edge(t.bx, t.by, t.cx, t.cy, px, py), wb = edge(t.cx, t.cy, t.ax, t.ay, px, py), wc = edge(t.ax, t.ay, t.bx, t.by, px, py);
    const bool covered = t.area > 0.f ? (wa >= 0.f && wb >= 0.f && wc >= 0.f) : (wa <= 0.f && wb <= 0.f && wc <= 0.f);
    if (!covered) return;
    const float z = t.area / (wa * t.qa + wb * t.qb + wc * t.qc);
    if (!(z > 0.f && z < __uint_as_float(INF_BITS))) return;
    unsigned* p = zb + (size_t)j * W + i;
    const unsigned bits = __float_as_uint(z);
    if (bits < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, bits);
}

__global__ __launch_bounds__(THREADS) void cull_raster(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                       long long n_f, const float* __restrict__ K, const float* __restrict__ poses,
                                                       long long cam0, int nc, int W, int H, float near_distance, unsigned* zbuf) {
    __shared__ float s_cam[12 * CAM_TILE];
    load_cameras(poses, cam0, nc, s_cam);
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    int idx[3];
    const bool valid = f < n_f && load_face(faces, f, (unsigned)n_v, idx);
    float x[3][3] = {};
    if (valid) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* p = vertices + 3 * (size_t)idx[k];
            x[k][0] = p[0];
            x[k][1] = p[1];
            x[k][2] = p[2];
        }
    }
    const Intrinsics in = load_intrinsics(K);
    const int lane = threadIdx.x & 63;
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    for (int ci = 0; ci < nc; ++ci) {                   // wave-uniform: every lane takes part in the ballots below
        const float* o = s_cam + 12 * ci;
        unsigned* zb = zbuf + (size_t)ci * H * W;
        Tri t;
        float da, db, dc;
        project(o, in, x[0][0], x[0][1], x[0][2], t.ax, t.ay, da);
        project(o, in, x[1][0], x[1][1], x[1][2], t.bx, t.by, db);
        project(o, in, x[2][0], x[2][1], x[2][2], t.cx, t.cy, dc);
        t.qa = 1.0f / da;
        t.qb = 1.0f / db;
        t.qc = 1.0f / dc;
        t.area = edge(t.ax, t.ay, t.bx, t.by, t.cx, t.cy);
        bool ok = valid && da >= near_distance && db >= near_distance && dc >= near_distance;
        ok = ok && t.area != 0.f && fabsf(t.area) < __uint_as_float(INF_BITS);
        const float fi0 = fmaxf(0.f, floorf(fminf(fminf(t.ax, t.bx), t.cx))), fi1 = fminf(wmax, floorf(fmaxf(fmaxf(t.ax, t.bx), t.cx)));
        const float fj0 = fmaxf(0.f, floorf(fminf(fminf(t.ay, t.by), t.cy))), fj1 = fminf(hmax, floorf(fmaxf(fmaxf(t.ay, t.by), t.cy)));
        ok = ok && fi0 <= fi1 && fj0 <= fj1;
        t.i0 = ok ? (int)fi0 : 0;                       // inside [0, W - 1] x [0, H - 1] when ok
        t.i1 = ok ? (int)fi1 : -1;
        t.j0 = ok ? (int)fj0 : 0;
        t.j1 = ok ? (int)fj1 : -1;
        const bool big = ok && (t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1) > SMALL_BOX;
        if (ok && !big) {
            for (int j = t.j0; j <= t.j1; ++j)
                for (int i = t.i0; i <= t.i1; ++i) shade(t, i, j, zb, W);
        }
        unsigned long long todo = __ballot(big);
        while (todo) {                                  // the wave walks each large box together
            const int leader = __ffsll((long long)todo) - 1;
            Tri w;
            w.ax = __shfl(t.ax, leader, 64);
            w.ay = __shfl(t.ay, leader, 64);
            w.bx = __shfl(t.bx, leader, 64);
            w.by = __shfl(t.by, leader, 64);
            w.cx = __shfl(t.cx, leader, 64);
            w.cy = __shfl(t.cy, leader, 64);
            w.qa = __shfl(t.qa, leader, 64);
            w.qb = __shfl(t.qb, leader, 64);
            w.qc = __shfl(t.qc, leader, 64);
            w.area = __shfl(t.area, leader, 64);
            w.i0 = __shfl(t.i0, leader, 64);
            w.i1 = __shfl(t.i1, leader, 64);
            w.j0 = __shfl(t.j0, leader, 64);
            w.j1 = __shfl(t.j1, leader, 64);
            for (int j = w.j0 + (lane >> 3); j <= w.j1; j += 8)
                for (int i = w.i0 + (lane & 7); i <= w.i1; i += 8) shade(w, i, j, zb, W);
            todo &= todo - 1;
        }
    }
}

__global__ __launch_bounds__(THREADS) void cull_test(const float* __restrict__ vertices, long long n_v, const float* __restrict__ K,
                                                     const float* __restrict__ poses, long long cam0, int nc, int W, int H,
                                                     float near_distance, float bias, const unsigned* __restrict__ zbuf,
                                                     int* __restrict__ vertex_views, int accumulate) {
    __shared__ float s_cam[12 * CAM_TILE];
    load_cameras(poses, cam0, nc, s_cam);
    const long long vi = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (vi >= n_v) return;
    const float x = vertices[3 * vi], y = vertices[3 * vi + 1], z = vertices[3 * vi + 2];
    const Intrinsics in = load_intrinsics(K);
    const float wf = (float)W, hf = (float)H;
    int views = 0;
    for (int ci = 0; ci < nc; ++ci) {
        float u, v, d;
        project(s_cam + 12 * ci, in, x, y, z, u, v, d);
        if (!(d >= near_distance && u >= 0.f && u < wf && v >= 0.f && v < hf)) continue;
        const int i = (int)floorf(u), j = (int)floorf(v);   // inside [0, W - 1] x [0, H - 1]
        const float nearest = __uint_as_float(zbuf[((size_t)ci * H + j) * W + i]);
        views += d <= nearest + bias;
    }
    vertex_views[vi] = accumulate ? vertex_views[vi] + views : views;
}

// the cull's rule: some vertex of the face has min_views views
struct ViewsKeep {
    const int* views;
    int min_views;
    __device__ bool operator()(const int v[3]) const { return views[v[0]] >= min_views || views[v[1]] >= min_views || views[v[2]] >= min_views; }
};

inline bool image_ok(int W, int H) { return W >= 1 && H >= 1 && W <= MAX_WH && H <= MAX_WH; }

}  // namespace

NGP_API int ngp_meshcull_abi_version(void) { return 1; }

NGP_API const char* ngp_meshcull_build_arch(void) { return "gfx950"; }

NGP_API size_t ngp_meshcull_zbuffer_bytes(int W, int H, int64_t n_cams) {
    if (!image_ok(W, H) || n_cams < 1 || n_cams > INT32_MAX) return 0;
    return (size_t)4 * W * H * (size_t)n_cams;
}

NGP_API size_t ngp_meshcull_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    if (!sizes_ok(n_vertices, n_faces)) return 0;
    return layout(n_vertices, n_faces).total;
}

NGP_API int ngp_meshcull_views(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, const float* K,
                               const float* poses, int64_t n_cams, int W, int H, float near_distance, float bias, void* zbuffer,
                               size_t zbuffer_bytes, int32_t* vertex_views, void* stream) {
    if (n_vertices < 0 || n_faces < 0 || n_cams < 1 || !image_ok(W, H)) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX || n_cams > INT32_MAX) return NGP_ERANGE;
    if (n_vertices == 0) return 0;
    if (!vertices || !K || !poses || !zbuffer || !vertex_views || (n_faces > 0 && !faces)) return NGP_EINVAL;
    const size_t pixels = (size_t)W * H;
    const size_t fit = zbuffer_bytes / (4 * pixels);
    if (fit < 1) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long n_v = n_vertices, n_f = n_faces;
    const unsigned vb = (unsigned)blocks_of(n_v, THREADS), fb = (unsigned)blocks_of(n_f, THREADS);
    unsigned* zbuf = (unsigned*)zbuffer;
    const long long chunk = (long long)(fit < (size_t)n_cams ? fit : (size_t)n_cams);
    for (long long c0 = 0; c0 < n_cams; c0 += chunk) {
        const long long in_chunk = n_cams - c0 < chunk ? n_cams - c0 : chunk;
        const hipError_t e = hipMemsetD32Async((hipDeviceptr_t)zbuf, (int)INF_BITS, (size_t)in_chunk * pixels, s);
        if (e != hipSuccess) return (int)e;
        for (long long t0 = 0; fb && t0 < in_chunk; t0 += CAM_TILE) {
            const int nc = (int)(in_chunk - t0 < CAM_TILE ? in_chunk - t0 : CAM_TILE);
            hipLaunchKernelGGL(cull_raster, dim3(fb), dim3(THREADS), 0, s, vertices, faces, n_v, n_f, K, poses, c0 + t0, nc, W, H,
                               near_distance, zbuf + (size_t)t0 * pixels);
        }
        for (long long t0 = 0; t0 < in_chunk; t0 += CAM_TILE) {
            const int nc = (int)(in_chunk - t0 < CAM_TILE ? in_chunk - t0 : CAM_TILE);
            hipLaunchKernelGGL(cull_test, dim3(vb), dim3(THREADS), 0, s, vertices, n_v, K, poses, c0 + t0, nc, W, H, near_distance, bias,
                               (const unsigned*)(zbuf + (size_t)t0 * pixels), vertex_views, (int)(c0 + t0 > 0));
        }
    }
    return launched();
}

NGP_API int ngp_meshcull_count(const int32_t* faces, const int32_t* vertex_views, int32_t min_views, int64_t n_vertices, int64_t n_faces,
                               void* workspace, size_t workspace_bytes, int64_t* totals, void* stream) {
    if (n_vertices < 0 || n_faces < 0) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (n_vertices == 0 && n_faces == 0) return 0;
    if (!workspace || !totals || (n_vertices > 0 && !vertex_views) || (n_faces > 0 && !faces)) return NGP_EINVAL;
    if (workspace_bytes < layout(n_vertices, n_faces).total) return NGP_EINVAL;
    return compact_count(ViewsKeep{vertex_views, min_views}, faces, n_vertices, n_faces, (char*)workspace, (long long*)totals, (hipStream_t)stream);
}

NGP_API int ngp_meshcull_emit(const int32_t* faces, const int32_t* vertex_views, int32_t min_views, const float* vertices,
                              const float* normals, const float* colors, int64_t n_vertices, int64_t n_faces, void* workspace,
                              size_t workspace_bytes, int64_t out_vertices, int64_t out_faces, float* vertices_out, float* normals_out,
                              float* colors_out, int32_t* faces_out, void* stream) {
    if (n_vertices < 0 || n_faces < 0 || out_vertices < 0 || out_faces < 0) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (out_vertices > n_vertices || out_faces > n_faces) return NGP_EINVAL;
    if (out_vertices == 0 && out_faces == 0) return 0;
    if (!workspace || !vertex_views || !faces) return NGP_EINVAL;
    if (out_vertices > 0 && (!vertices || !vertices_out || !normals != !normals_out || !colors != !colors_out)) return NGP_EINVAL;
    if (out_faces > 0 && !faces_out) return NGP_EINVAL;
    if (workspace_bytes < layout(n_vertices, n_faces).total) return NGP_EINVAL;
    return compact_emit(ViewsKeep{vertex_views, min_views}, faces, vertices, normals, colors, n_vertices, n_faces, (char*)workspace, out_vertices,
                        out_faces, vertices_out, normals_out, colors_out, faces_out, (hipStream_t)stream);
}
