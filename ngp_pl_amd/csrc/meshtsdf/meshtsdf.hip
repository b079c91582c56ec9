// libngp_meshtsdf.so: fusion of per-camera depth maps into a truncated signed distance volume on the export lattice (C ABI and the
// exact rule: include/ngp_meshtsdf.h).  Compiled with -ffp-contract=off: every f32 expression below is the header's, operation by
// operation.
//
//   tsdf_integrate   one thread per lattice point, x fastest: the 64 points of a wave are a piece of a lattice row (or of two) and
//                    project to a short pixel segment, so a wave's depth gather touches few lines.  The thread holds its point and
//                    its state (acc, seen, behind) in registers and walks ALL the cameras of the call in ascending order, tile by
//                    tile of CAM_TILE cameras whose R^T and -R^T t (camera_rows of ../mesh_camera.h, shared with the other camera
//                    stages; the projection body is this kernel's own) pass through LDS: the state is read once and written once per
//                    call, and a sequential per-thread sum needs no atomic.
//   tsdf_finish      one thread per point: the volume from the state (vol may be acc).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/ngp_meshtsdf.h"

namespace {

#include "../mesh_host.h"

constexpr int THREADS = 256;
constexpr int CAM_TILE = 128;                           // cameras per LDS tile: 12 floats each
constexpr int MAX_WH = 16384;
constexpr int MAX_AXIS = 65535;
constexpr long long MAX_POINTS = 1LL << 36;

struct Dims {
    int nx, ny, nz;
    long long n;
};

struct Geom {
    float lo[3], h[3];
};

#include "../mesh_camera.h"

// per camera of the tile: the 9 entries of R^T, then -R^T t (the header's m and s); the barriers are the caller's
__device__ inline void load_cameras(const float* __restrict__ poses, long long cam0, int nc, float* s_cam) {
    for (int i = threadIdx.x; i < nc; i += blockDim.x) camera_rows(poses + 12 * (size_t)(cam0 + i), s_cam + 12 * i);
}

__global__ __launch_bounds__(THREADS) void tsdf_integrate(Dims dm, Geom g, const float* __restrict__ K, const float* __restrict__ poses,
                                                          const float* __restrict__ depth, long long n_cams, int W, int H,
                                                          float near_distance, float trunc, float* __restrict__ acc_io,
                                                          int* __restrict__ seen_io, int* __restrict__ behind_io) {
    __shared__ float s_cam[12 * CAM_TILE];
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    const bool valid = p < dm.n;                        // every thread stays for the barriers of the tile loop
    float x = 0.f, y = 0.f, z = 0.f, acc = 0.f;
    int seen = 0, behind = 0;
    if (valid) {
        const unsigned long long row = (unsigned long long)p / (unsigned)dm.nx;
        const int i = (int)(p - (long long)row * dm.nx);
        const unsigned long long kk = row / (unsigned)dm.ny;
        const int k = (int)kk, j = (int)(row - kk * dm.ny);
        x = g.lo[0] + (float)i * g.h[0];
        y = g.lo[1] + (float)j * g.h[1];
        z = g.lo[2] + (float)k * g.h[2];
        acc = acc_io[p];
        seen = seen_io[p];
        behind = behind_io[p];
    }
    const Intrinsics in = load_intrinsics(K);
    const float wf = (float)W, hf = (float)H, minus_trunc = -trunc;
    const size_t pixels = (size_t)W * H;
    for (long long c0 = 0; c0 < n_cams; c0 += CAM_TILE) {
        const int nc = (int)(n_cams - c0 < CAM_TILE ? n_cams - c0 : CAM_TILE);
        __syncthreads();                                // the previous tile has been read by every wave
        load_cameras(poses, c0, nc, s_cam);
        __syncthreads();
        if (!valid) continue;
        const float* img = depth + (size_t)c0 * pixels;
        for (int ci = 0; ci < nc; ++ci, img += pixels) {
            const float* o = s_cam + 12 * ci;
            const float px = o[0] * x + o[1] * y + o[2] * z + o[9];
            const float py = o[3] * x + o[4] * y + o[5] * z + o[10];
            const float pz = o[6] * x + o[7] * y + o[8] * z + o[11];
            const float d = in.k[6] * px + in.k[7] * py + in.k[8] * pz;
            if (!(d >= near_distance)) continue;
            const float ud = in.k[0] * px + in.k[1] * py + in.k[2] * pz, vd = in.k[3] * px + in.k[4] * py + in.k[5] * pz;
            const float u = ud / d, v = vd / d;
            if (!(u >= 0.f && u < wf && v >= 0.f && v < hf)) continue;
            const int iu = (int)floorf(u), iv = (int)floorf(v);     // inside [0, W - 1] x [0, H - 1]
            const float D = img[(size_t)iv * W + iu];
            if (!(D > 0.f)) continue;
            const float sdf = D - d;
            if (sdf < minus_trunc) {
                ++behind;
            } else {
                const float q = sdf / trunc;
                acc = acc + (q < 1.f ? q : 1.f);
                ++seen;
            }
        }
    }
    if (valid) {
        acc_io[p] = acc;
        seen_io[p] = seen;
        behind_io[p] = behind;
    }
}

// vol may alias acc: each thread reads its own element before it writes it
__global__ __launch_bounds__(THREADS) void tsdf_finish(long long n, const float* acc, const int* __restrict__ seen,
                                                       const int* __restrict__ behind, float* vol) {
    const long long p = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (p >= n) return;
    const int s = seen[p];
    vol[p] = s > 0 ? -(acc[p] / (float)s) : (behind[p] > 0 ? 1.f : -1.f);
}

bool dims_ok(int nx, int ny, int nz, Dims& d) {
    if (nx < 2 || ny < 2 || nz < 2 || nx > MAX_AXIS || ny > MAX_AXIS || nz > MAX_AXIS) return false;
    d.nx = nx;
    d.ny = ny;
    d.nz = nz;
    d.n = (long long)nx * ny * nz;
    return d.n <= MAX_POINTS;
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

NGP_API int ngp_meshtsdf_abi_version(void) { return 1; }

NGP_API const char* ngp_meshtsdf_build_arch(void) { return "gfx950"; }

NGP_API size_t ngp_meshtsdf_state_bytes(int nx, int ny, int nz) {
    Dims d;
    if (!dims_ok(nx, ny, nz, d)) return 0;
    return (size_t)12 * (size_t)d.n;
}

NGP_API int ngp_meshtsdf_integrate(int nx, int ny, int nz, const float* bounds6, const float* K, const float* poses, const float* depth,
                                   int64_t n_cams, int W, int H, float near_distance, float trunc, float* acc, int32_t* seen,
                                   int32_t* behind, void* stream) {
    Dims d;
    Geom g;
    if (!dims_ok(nx, ny, nz, d) || !bounds6 || !K || !poses || !depth || !acc || !seen || !behind) return NGP_EINVAL;
    if (n_cams < 1 || W < 1 || H < 1 || W > MAX_WH || H > MAX_WH) return NGP_EINVAL;
    if (!(trunc > 0.f) || !(trunc < 3.0e38f) || !geom_ok(d, bounds6, g)) return NGP_EINVAL;     // NaN and infinities fail
    if (n_cams > INT32_MAX) return NGP_ERANGE;
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((d.n + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(tsdf_integrate, dim3(blocks), dim3(THREADS), 0, s, d, g, K, poses, depth, (long long)n_cams, W, H, near_distance,
                       trunc, acc, (int*)seen, (int*)behind);
    return launched();
}

NGP_API int ngp_meshtsdf_finish(int64_t n_points, const float* acc, const int32_t* seen, const int32_t* behind, float* vol, void* stream) {
    if (n_points < 0 || n_points > MAX_POINTS) return NGP_EINVAL;
    if (n_points == 0) return 0;
    if (!acc || !seen || !behind || !vol) return NGP_EINVAL;
    const unsigned blocks = (unsigned)((n_points + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(tsdf_finish, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, (long long)n_points, acc, (const int*)seen,
                       (const int*)behind, vol);
    return launched();
}
