// libngp_meshcull.so: depth-buffer visibility of an indexed triangle mesh against pinhole cameras, and the sub-mesh of the faces
// some camera sees (C ABI and the exact rule: include/ngp_meshcull.h).  Compiled with -ffp-contract=off: every f32 expression
// below is the header's, operation by operation.
//
// Views, per chunk of as many cameras as the caller's depth workspace holds, on the caller's stream:
//   clear            the chunk's buffers to the bits of +inf (hipMemsetD32Async);
//   cull_raster      the shared rasteriser of ../mesh_raster.h (one work item per (face, camera), at most CAM_TILE cameras per
//                    launch, a lane walker for small pixel boxes and a wave walker for large ones) with the sink DepthSink:
//                    atomicMin on the depth's bits, skipped when an L2 read of the pixel already holds a smaller or equal depth
//                    (the buffer only ever falls, so a skipped write is never missed);
//   cull_test        one thread per vertex walks the same cameras (../mesh_camera.h) and adds the views it has: a plain
//                    per-vertex sum, no atomic.
// Compaction is the shared one of ../mesh_compact.h with the rule ViewsKeep (a face is kept iff a vertex of it has min_views views).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/ngp_meshcull.h"

namespace {

#include "../mesh_compact.h"                           // THREADS and load_face, which mesh_raster.h expects
#include "../mesh_camera.h"
#include "../mesh_raster.h"

constexpr int MAX_WH = 16384;
constexpr unsigned INF_BITS = 0x7F800000u;

// per camera of the launch: the 9 entries of R^T, then -R^T t (the header's m and s)
__device__ inline void load_cameras(const float* __restrict__ poses, long long cam0, int nc, float* s_cam) {
    for (int i = threadIdx.x; i < nc; i += blockDim.x) camera_rows(poses + 12 * (size_t)(cam0 + i), s_cam + 12 * i);
    __syncthreads();
}

__global__ __launch_bounds__(THREADS) void cull_raster(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                       long long n_f, const float* __restrict__ K, const float* __restrict__ poses,
                                                       long long cam0, int nc, int W, int H, float near_distance, unsigned* zbuf) {
    raster_faces(DepthSink{}, vertices, faces, n_v, n_f, K, poses, cam0, nc, W, H, near_distance, zbuf);
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
