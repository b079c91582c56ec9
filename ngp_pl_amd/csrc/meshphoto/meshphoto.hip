// libngp_meshphoto.so: the colour of surface points blended from photographs with known cameras (C ABI and the exact rule:
// ngp_meshphoto.h, beside this file).  Compiled with -ffp-contract=off: every f32 expression below is the header's, operation by
// operation.
//
//   photo_accumulate one thread per point; the 64 points of a wave are consecutive texels of an atlas row, which lie side by side
//                    on a face, project to neighbouring pixels and so gather their depths and their colours from the same few
//                    cache lines.  The thread holds its point, its direction and its sums (acc[4], views) in registers and walks
//                    ALL the cameras of the call in ascending order, tile by tile of CAM_TILE cameras whose R^T, -R^T t (camera_rows
//                    of ../mesh_camera.h, shared with the other camera stages; the projection body is this kernel's own) and t
//                    pass through LDS (every lane reads the same address: a broadcast): the sums are read once and written once
//                    per call, and a sequential per-thread sum needs no atomic.  Per camera the cheap rejects (depth, frame,
//                    viewing angle: tests 1 to 3, registers only) come first; a wave whose ballot shows no lane left skips the
//                    camera's window of depths and its colours entirely, which is the common case: a texel row faces away from
//                    half the cameras and is outside the frame of others.  K is the same for every thread: scalar loads.
//   photo_resolve    one thread per point: rgb and seen from the sums.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngp_meshphoto.h"

namespace {

#include "../mesh_host.h"

constexpr int THREADS = 256;
constexpr int CAM_TILE = 64;                            // cameras per LDS tile: CAM_FLOATS floats each (4 KiB)
constexpr int CAM_FLOATS = 16;                          // m (9), s (3), o (3), one of padding: a camera starts on a 64-byte line
constexpr int MAX_WH = 16384;
constexpr unsigned INF_BITS = 0x7F800000u;

#include "../mesh_camera.h"

struct Params {
    int W, H, guard, power;
    float near_distance, bias, min_cos;
};

__device__ inline bool finite(float x) { return fabsf(x) < __uint_as_float(INF_BITS); }        // false for NaN

// per camera of the tile: the 9 entries of R^T, then -R^T t (the header's m and s), then t (the header's o)
__device__ inline void load_cameras(const float* __restrict__ poses, long long cam0, int nc, float* s_cam) {
    for (int i = threadIdx.x; i < nc; i += blockDim.x) {
        const float* P = poses + 12 * (size_t)(cam0 + i);   // row-major 3 x 4: [R | t]
        float* o = s_cam + CAM_FLOATS * i;
        camera_rows(P, o);
        o[12] = P[3];
        o[13] = P[7];
        o[14] = P[11];
        o[15] = 0.f;
    }
}

// test 4 of the rule: every depth of the guard window round pixel (ic, jc), which lies inside the image, within bias of d
__device__ inline bool window_agrees(const unsigned* __restrict__ zb, int W, int H, int ic, int jc, int guard, float d, float bias) {
    const int i_lo = max(ic - guard, 0), i_hi = min(ic + guard, W - 1), j_lo = max(jc - guard, 0), j_hi = min(jc + guard, H - 1);
    bool ok = true;
    for (int j = j_lo; j <= j_hi && ok; ++j) {
        const unsigned* row = zb + (size_t)j * W;
        for (int i = i_lo; i <= i_hi; ++i) {
            const float z = __uint_as_float(row[i]);
            ok = ok && d <= z + bias && z <= d + bias;
        }
    }
    return ok;
}

__global__ __launch_bounds__(THREADS) void photo_accumulate(const float* __restrict__ points, const float* __restrict__ dirs,
                                                            const uint8_t* __restrict__ valid, long long n, const float* __restrict__ K,
                                                            const float* __restrict__ poses, long long n_cams,
                                                            const uint8_t* __restrict__ images, const unsigned* __restrict__ zbuf, Params pr,
                                                            float* __restrict__ acc_io, int* __restrict__ views_io) {
    __shared__ float s_cam[CAM_FLOATS * CAM_TILE];
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    float x0 = 0.f, x1 = 0.f, x2 = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f;
    bool live = false;                                  // every thread stays for the barriers and the ballots of the tile loop
    if (p < n && valid[p] != 0) {
        x0 = points[3 * p];
        x1 = points[3 * p + 1];
        x2 = points[3 * p + 2];
        g0 = dirs[3 * p];
        g1 = dirs[3 * p + 1];
        g2 = dirs[3 * p + 2];
        live = finite(x0) && finite(x1) && finite(x2) && finite(g0) && finite(g1) && finite(g2);
    }
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int views = 0;
    if (live) {
        const float4 a = *reinterpret_cast<const float4*>(acc_io + 4 * p);
        a0 = a.x;
        a1 = a.y;
        a2 = a.z;
        a3 = a.w;
        views = views_io[p];
    }
    const Intrinsics in = load_intrinsics(K);
    const int W = pr.W, H = pr.H;
    const float u_max = (float)W - 0.5f, v_max = (float)H - 0.5f;
    const size_t pixels = (size_t)W * H;
    for (long long c0 = 0; c0 < n_cams; c0 += CAM_TILE) {
        const int nc = (int)(n_cams - c0 < CAM_TILE ? n_cams - c0 : CAM_TILE);
        __syncthreads();                                // the previous tile has been read by every wave
        load_cameras(poses, c0, nc, s_cam);
        __syncthreads();
        for (int ci = 0; ci < nc; ++ci) {               // wave-uniform: every lane takes part in the ballot
            const float* o = s_cam + CAM_FLOATS * ci;
            const float px = o[0] * x0 + o[1] * x1 + o[2] * x2 + o[9];
            const float py = o[3] * x0 + o[4] * x1 + o[5] * x2 + o[10];
            const float pz = o[6] * x0 + o[7] * x1 + o[8] * x2 + o[11];
            const float d = in.k[6] * px + in.k[7] * py + in.k[8] * pz;
            const float ud = in.k[0] * px + in.k[1] * py + in.k[2] * pz, vd = in.k[3] * px + in.k[4] * py + in.k[5] * pz;
            const float u = ud / d, v = vd / d;
            const float e0 = o[12] - x0, e1 = o[13] - x1, e2 = o[14] - x2;
            const float L = sqrtf((e0 * e0 + e1 * e1) + e2 * e2);
            const float cs = -((g0 * e0 + g1 * e1) + g2 * e2) / L;
            const bool cheap = live && d >= pr.near_distance && u >= 0.5f && u <= u_max && v >= 0.5f && v <= v_max && L > 0.f &&
                               cs >= pr.min_cos;
            if (__ballot(cheap) == 0ull) continue;      // nobody in this wave reads this camera
            if (!cheap) continue;
            // u in [0.5, W - 0.5] and v in [0.5, H - 0.5]: every index below lies inside the image
            const size_t cam = (size_t)(c0 + ci);
            if (!window_agrees(zbuf + cam * pixels, W, H, (int)floorf(u), (int)floorf(v), pr.guard, d, pr.bias)) continue;
            const float X = u - 0.5f, Y = v - 0.5f;
            const float flx = floorf(X), fly = floorf(Y);
            const int i0 = (int)flx, j0 = (int)fly;
            const float fx = X - flx, fy = Y - fly;
            const int i1 = min(i0 + 1, W - 1), j1 = min(j0 + 1, H - 1);
            const uint8_t* img = images + cam * pixels * 3;
            const uint8_t* t00 = img + ((size_t)j0 * W + i0) * 3;
            const uint8_t* t10 = img + ((size_t)j0 * W + i1) * 3;
            const uint8_t* t01 = img + ((size_t)j1 * W + i0) * 3;
            const uint8_t* t11 = img + ((size_t)j1 * W + i1) * 3;
            float w = cs;
            for (int k = 1; k < pr.power; ++k) w = w * cs;
            const float gx = 1.f - fx, gy = 1.f - fy;
            float col[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float top = (float)t00[k] * gx + (float)t10[k] * fx;
                const float bot = (float)t01[k] * gx + (float)t11[k] * fx;
                col[k] = top * gy + bot * fy;
            }
            a0 = a0 + w * col[0];
            a1 = a1 + w * col[1];
            a2 = a2 + w * col[2];
            a3 = a3 + w;
            ++views;
        }
    }
    if (live) {
        *reinterpret_cast<float4*>(acc_io + 4 * p) = make_float4(a0, a1, a2, a3);
        views_io[p] = views;
    }
}

__global__ __launch_bounds__(THREADS) void photo_resolve(const float* __restrict__ acc, const int* __restrict__ views,
                                                         const uint8_t* __restrict__ valid, long long n, int min_views,
                                                         float* __restrict__ rgb, uint8_t* __restrict__ seen) {
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (p >= n) return;
    const float4 a = *reinterpret_cast<const float4*>(acc + 4 * p);
    const bool ok = valid[p] != 0 && views[p] >= min_views && a.w > 0.f;
    rgb[3 * p] = ok ? (a.x / a.w) / 255.f : 0.f;
    rgb[3 * p + 1] = ok ? (a.y / a.w) / 255.f : 0.f;
    rgb[3 * p + 2] = ok ? (a.z / a.w) / 255.f : 0.f;
    seen[p] = ok ? 1 : 0;
}

inline bool host_finite(float x) { return x - x == 0.f; }

}  // namespace

NGP_API int ngp_meshphoto_abi_version(void) { return 1; }

NGP_API const char* ngp_meshphoto_build_arch(void) { return "gfx950"; }

NGP_API int ngp_meshphoto_accumulate(const float* points, const float* dirs, const uint8_t* valid, int64_t n, const float* K,
                                     const float* poses, int64_t n_cams, int W, int H, const uint8_t* images, const uint32_t* zbuf,
                                     float near_distance, float bias, int guard, float min_cos, int power, float* acc, int32_t* views,
                                     void* stream) {
    if (n < 0 || n_cams < 1 || W < 1 || H < 1 || W > MAX_WH || H > MAX_WH) return NGP_EINVAL;
    if (guard < 0 || guard > NGP_MESHPHOTO_MAX_GUARD || power < 1 || power > NGP_MESHPHOTO_MAX_POWER) return NGP_EINVAL;
    if (!host_finite(near_distance) || !host_finite(bias) || !(bias >= 0.f) || !(min_cos > 0.f) || !(min_cos <= 1.f)) return NGP_EINVAL;   // NaN fails
    if (n > INT32_MAX || n_cams > INT32_MAX) return NGP_ERANGE;
    if (n == 0) return 0;
    if (!points || !dirs || !valid || !K || !poses || !images || !zbuf || !acc || !views) return NGP_EINVAL;
    if (((uintptr_t)acc & 15) || ((uintptr_t)zbuf & 3) || ((uintptr_t)views & 3)) return NGP_EINVAL;   // acc is read and written as float4
    Params pr;
    pr.W = W;
    pr.H = H;
    pr.guard = guard;
    pr.power = power;
    pr.near_distance = near_distance;
    pr.bias = bias;
    pr.min_cos = min_cos;
    const unsigned blocks = (unsigned)((n + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(photo_accumulate, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, points, dirs, valid, (long long)n, K, poses,
                       (long long)n_cams, images, (const unsigned*)zbuf, pr, acc, (int*)views);
    return launched();
}

NGP_API int ngp_meshphoto_resolve(const float* acc, const int32_t* views, const uint8_t* valid, int64_t n, int32_t min_views, float* rgb,
                                  uint8_t* seen, void* stream) {
    if (n < 0 || min_views < 1) return NGP_EINVAL;
    if (n > INT32_MAX) return NGP_ERANGE;
    if (n == 0) return 0;
    if (!acc || !views || !valid || !rgb || !seen || ((uintptr_t)acc & 15)) return NGP_EINVAL;
    const unsigned blocks = (unsigned)((n + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(photo_resolve, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, acc, (const int*)views, valid, (long long)n,
                       (int)min_views, rgb, seen);
    return launched();
}
