// libngp_meshtex.so: a texture atlas for an indexed triangle mesh and a renderer of the textured mesh against pinhole cameras (C ABI
// and the exact rule: include/ngp_meshtex.h).  Compiled with -ffp-contract=off: every f32 expression below is the header's,
// operation by operation.
//
//   tex_points   one thread per texel of the caller's range: row and column of the atlas, cell and local texel (one division by
//                CW and one by CH per thread), slot, face, the three vertices and normals; consecutive texels of a row share one
//                or two faces, so the loads of a wave fall on a few lines.
//   tex_uvs      one thread per face: six f64 expressions.
//   Render, per chunk of as many cameras as the caller's workspace holds, on the caller's stream:
//   clear        the chunk's keys to all ones (hipMemsetAsync);
//   tex_raster   the shared rasteriser of ../mesh_raster.h (one work item per (face, camera), at most CAM_TILE cameras per launch,
//                a lane walker for small pixel boxes and a wave walker for large ones) with the sink KeySink: the 64-bit atomic
//                minimum of (depth bits, face), skipped when a read of the pixel already holds a smaller key (a key only ever
//                falls, so a skipped write is never missed);
//   tex_shade    one thread per pixel: the winning face re-projected as the raster projected it and the bilinear lookup in the
//                atlas, both of ../mesh_raster.h; between them this library's own mapping from (face, beta, gamma) to the atlas.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../../include/ngp_meshtex.h"

namespace {

#include "../mesh_host.h"

constexpr int THREADS = 256;
constexpr int MAX_WH = 16384;
constexpr int MAX_TEXELS = 256;
constexpr float INF = __builtin_inff();
constexpr unsigned long long NO_KEY = ~0ull;

struct Atlas {
    int T, cw, ch, c, W, H;
    long long n_cells;
};

// the header's layout; 0, NGP_EINVAL or NGP_ERANGE
inline int atlas_layout(int64_t n_faces, int texels, Atlas& a) {
    if (n_faces < 1 || texels < 1 || texels > MAX_TEXELS) return NGP_EINVAL;
    if (n_faces > INT32_MAX) return NGP_ERANGE;
    a.T = texels;
    a.cw = texels + 5;
    a.ch = texels + 4;
    a.n_cells = (n_faces + 1) / 2;
    for (long long c = 1; c * a.cw <= MAX_WH; ++c) {
        const long long rows = (a.n_cells + c - 1) / c;
        if (c * a.cw >= rows * a.ch) {                  // then rows * ch <= c * cw <= MAX_WH as well
            a.c = (int)c;
            a.W = (int)(c * a.cw);
            a.H = (int)(rows * a.ch);
            return 0;
        }
    }
    return NGP_ERANGE;
}

inline bool finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

inline bool image_ok(int W, int H) { return W >= 1 && H >= 1 && W <= MAX_WH && H <= MAX_WH; }

struct Box {
    float lo[3], hi[3];
};

__device__ inline bool load_face(const int* __restrict__ faces, long long f, unsigned n_v, int idx[3]) {
    idx[0] = faces[3 * f];
    idx[1] = faces[3 * f + 1];
    idx[2] = faces[3 * f + 2];
    return (unsigned)idx[0] < n_v && (unsigned)idx[1] < n_v && (unsigned)idx[2] < n_v;
}

__device__ inline bool finite(float x) { return fabsf(x) < INF; }   // false for NaN

__global__ __launch_bounds__(THREADS) void tex_points(const float* __restrict__ vertices, const int* __restrict__ faces,
                                                      const float* __restrict__ normals, long long n_v, long long n_f, Atlas a, Box box,
                                                      long long begin, long long count, float* __restrict__ points,
                                                      float* __restrict__ dirs, uint8_t* __restrict__ valid) {
    const long long k = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (k >= count) return;
    const int g = (int)(begin + k);                     // an atlas has at most 2^28 texels
    const int row = g / a.W, col = g - row * a.W;
    const int cy = row / a.ch, cx = col / a.cw;
    const int j = row - cy * a.ch, i = col - cx * a.cw;
    const long long cell = (long long)cy * a.c + cx;
    const bool slot1 = i + j > a.T + 3;
    const int is = slot1 ? a.T + 4 - i : i, js = slot1 ? a.T + 3 - j : j;
    const long long f = 2 * cell + (slot1 ? 1 : 0);
    float p[3] = {box.lo[0], box.lo[1], box.lo[2]}, d[3] = {0.f, 0.f, 1.f};
    bool ok = false;
    int idx[3];
    if (cell < a.n_cells && f < n_f && load_face(faces, f, (unsigned)n_v, idx)) {
        const float u = (float)(is - 1) / (float)a.T, v = (float)(js - 1) / (float)a.T;
        const float *A = vertices + 3 * (size_t)idx[0], *B = vertices + 3 * (size_t)idx[1], *C = vertices + 3 * (size_t)idx[2];
        float q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = (A[c] + u * (B[c] - A[c])) + v * (C[c] - A[c]);
        ok = finite(q[0]) && finite(q[1]) && finite(q[2]);
        if (ok) {
            const float *NA = normals + 3 * (size_t)idx[0], *NB = normals + 3 * (size_t)idx[1], *NC = normals + 3 * (size_t)idx[2];
            float n[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                p[c] = fminf(fmaxf(q[c], box.lo[c]), box.hi[c]);
                n[c] = (NA[c] + u * (NB[c] - NA[c])) + v * (NC[c] - NA[c]);
            }
            const float L = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            const float e0 = -(n[0] / L), e1 = -(n[1] / L), e2 = -(n[2] / L);
            if (L > 0.f && finite(e0) && finite(e1) && finite(e2)) {
                d[0] = e0;
                d[1] = e1;
                d[2] = e2;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        points[3 * (size_t)k + c] = p[c];
        dirs[3 * (size_t)k + c] = d[c];
    }
    valid[k] = ok ? 1 : 0;
}

// the atlas texel of the corner at slot coordinates (is, js) of face f
__device__ inline void corner_texel(const Atlas& a, long long f, int is, int js, int& gi, int& gj) {
    const long long cell = f >> 1;
    const int cy = (int)(cell / a.c), cx = (int)(cell - (long long)cy * a.c);
    const bool slot1 = (f & 1) != 0;
    gi = cx * a.cw + (slot1 ? a.T + 4 - is : is);
    gj = cy * a.ch + (slot1 ? a.T + 3 - js : js);
}

__global__ __launch_bounds__(THREADS) void tex_uvs(long long n_f, Atlas a, float* __restrict__ uvs) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_f) return;
    const int is[3] = {1, 1 + a.T, 1}, js[3] = {1, 1, 1 + a.T};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int gi, gj;
        corner_texel(a, f, is[k], js[k], gi, gj);
        uvs[6 * (size_t)f + 2 * k] = (float)(((double)gi + 0.5) / (double)a.W);
        uvs[6 * (size_t)f + 2 * k + 1] = (float)(1.0 - ((double)gj + 0.5) / (double)a.H);
    }
}

// ---- render -----------------------------------------------------------------------------------------------------------------

#include "../mesh_camera.h"
#include "../mesh_raster.h"

__global__ __launch_bounds__(THREADS) void tex_raster(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                      long long n_f, const float* __restrict__ K, const float* __restrict__ poses,
                                                      long long cam0, int nc, int W, int H, float near_distance,
                                                      unsigned long long* keys) {
    raster_faces(KeySink{}, vertices, faces, n_v, n_f, K, poses, cam0, nc, W, H, near_distance, keys);
}

// grid: (blocks over H * W, cameras of the launch)
__global__ __launch_bounds__(THREADS) void tex_shade(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                     long long n_f, Atlas a, const uint8_t* __restrict__ texture,
                                                     const float* __restrict__ K, const float* __restrict__ poses, long long cam0,
                                                     long long out0, int W, int H, float bg0, float bg1, float bg2,
                                                     const unsigned long long* __restrict__ keys, float* __restrict__ image,
                                                     int* __restrict__ face_index, float* __restrict__ depth) {
    const int pix = blockIdx.x * THREADS + threadIdx.x;   // W * H <= 2^28
    if (pix >= W * H) return;
    const int ci = blockIdx.y;
    const size_t in_px = (size_t)ci * H * W + pix, out_px = (size_t)(out0 + ci) * H * W + pix;
    const unsigned long long key = keys[in_px];
    float rgb[3] = {bg0, bg1, bg2}, z = INF;
    int face = -1;
    const unsigned kf = (unsigned)(key & 0xFFFFFFFFull);
    int idx[3];
    if (key != NO_KEY && kf < (unsigned long long)n_f && load_face(faces, kf, (unsigned)n_v, idx)) {   // a key only ever names a face the raster accepted
        face = (int)kf;
        z = __uint_as_float((unsigned)(key >> 32));
        float beta, gamma;
        winner_weights(vertices, idx, K, poses + 12 * (size_t)(cam0 + ci), pix, W, beta, gamma);
        const float xs = 1.0f + beta * (float)a.T, ys = 1.0f + gamma * (float)a.T;
        const long long cell = (long long)(kf >> 1);
        const int cy = (int)(cell / a.c), cx = (int)(cell - (long long)cy * a.c);
        const float ox = (float)(cx * a.cw), oy = (float)(cy * a.ch);
        const bool slot1 = (kf & 1u) != 0;
        // X lies in [ox + 1, ox + T + 3] and Y in [oy + 1, oy + T + 2]: inside the face's own cell
        const float X = slot1 ? ox + ((float)(a.T + 4) - xs) : ox + xs;
        const float Y = slot1 ? oy + ((float)(a.T + 3) - ys) : oy + ys;
        atlas_bilinear(texture, a.W, a.H, X, Y, rgb);
    }
    image[3 * out_px] = rgb[0];
    image[3 * out_px + 1] = rgb[1];
    image[3 * out_px + 2] = rgb[2];
    if (face_index) face_index[out_px] = face;
    if (depth) depth[out_px] = z;
}

}  // namespace

NGP_API int ngp_meshtex_abi_version(void) { return 1; }

NGP_API const char* ngp_meshtex_build_arch(void) { return "gfx950"; }

NGP_API int ngp_meshtex_atlas_size(int64_t n_faces, int texels, int* cells_per_row, int* width, int* height) {
    if (!cells_per_row || !width || !height) return NGP_EINVAL;
    Atlas a;
    const int rc = atlas_layout(n_faces, texels, a);
    if (rc) return rc;
    *cells_per_row = a.c;
    *width = a.W;
    *height = a.H;
    return 0;
}

NGP_API int ngp_meshtex_texel_points(const float* vertices, const int32_t* faces, const float* normals, int64_t n_vertices, int64_t n_faces,
                                     int texels, const float* box, int64_t begin, int64_t count, float* points, float* dirs,
                                     uint8_t* valid, void* stream) {
    if (n_vertices < 0 || begin < 0 || count < 0) return NGP_EINVAL;
    Atlas a;
    const int rc = atlas_layout(n_faces, texels, a);
    if (rc) return rc;
    if (n_vertices > INT32_MAX) return NGP_ERANGE;
    const long long total = (long long)a.W * a.H;
    if (!box || begin > total || count > total - begin) return NGP_EINVAL;
    if (!finite3(box) || !finite3(box + 3) || !(box[0] <= box[3] && box[1] <= box[4] && box[2] <= box[5])) return NGP_EINVAL;
    if (count == 0) return 0;                           // nothing to write: the outputs may be empty
    if (!faces || !points || !dirs || !valid || (n_vertices > 0 && (!vertices || !normals))) return NGP_EINVAL;
    Box b;
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = box[k];
        b.hi[k] = box[3 + k];
    }
    hipLaunchKernelGGL(tex_points, dim3((unsigned)blocks_of(count, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, vertices, faces, normals,
                       (long long)n_vertices, (long long)n_faces, a, b, (long long)begin, (long long)count, points, dirs, valid);
    return launched();
}

NGP_API int ngp_meshtex_face_uvs(int64_t n_faces, int texels, float* uvs, void* stream) {
    Atlas a;
    const int rc = atlas_layout(n_faces, texels, a);
    if (rc) return rc;
    if (!uvs) return NGP_EINVAL;
    hipLaunchKernelGGL(tex_uvs, dim3((unsigned)blocks_of(n_faces, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, (long long)n_faces, a, uvs);
    return launched();
}

NGP_API size_t ngp_meshtex_render_workspace_bytes(int W, int H, int64_t n_cams) {
    if (!image_ok(W, H) || n_cams < 1 || n_cams > INT32_MAX) return 0;
    return (size_t)8 * W * H * (size_t)n_cams;
}

NGP_API int ngp_meshtex_render(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, int texels,
                               const uint8_t* texture, const float* K, const float* poses, int64_t n_cams, int W, int H,
                               float near_distance, const float* background, void* workspace, size_t workspace_bytes, float* image,
                               int32_t* face_index, float* depth, void* stream) {
    if (n_vertices < 0 || n_cams < 1 || !image_ok(W, H)) return NGP_EINVAL;
    Atlas a;
    const int rc = atlas_layout(n_faces, texels, a);
    if (rc) return rc;
    if (n_vertices > INT32_MAX || n_cams > INT32_MAX) return NGP_ERANGE;
    if (!faces || !texture || !K || !poses || !background || !workspace || !image || (n_vertices > 0 && !vertices)) return NGP_EINVAL;
    if (((uintptr_t)workspace & 7) != 0) return NGP_EINVAL;
    if (!isfinite(near_distance) || !finite3(background)) return NGP_EINVAL;
    const size_t pixels = (size_t)W * H;
    const size_t fit = workspace_bytes / (8 * pixels);
    if (fit < 1) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long n_v = n_vertices, n_f = n_faces;
    const unsigned fb = (unsigned)blocks_of(n_f, THREADS), pb = (unsigned)blocks_of((long long)pixels, THREADS);
    unsigned long long* keys = (unsigned long long*)workspace;
    const long long chunk = (long long)(fit < (size_t)n_cams ? fit : (size_t)n_cams);
    for (long long c0 = 0; c0 < n_cams; c0 += chunk) {
        const long long in_chunk = n_cams - c0 < chunk ? n_cams - c0 : chunk;
        const hipError_t e = hipMemsetAsync(keys, 0xFF, (size_t)in_chunk * pixels * 8, s);
        if (e != hipSuccess) return (int)e;
        for (long long t0 = 0; t0 < in_chunk; t0 += CAM_TILE) {
            const int nc = (int)(in_chunk - t0 < CAM_TILE ? in_chunk - t0 : CAM_TILE);
            hipLaunchKernelGGL(tex_raster, dim3(fb), dim3(THREADS), 0, s, vertices, faces, n_v, n_f, K, poses, c0 + t0, nc, W, H, near_distance,
                               keys + (size_t)t0 * pixels);
        }
        for (long long t0 = 0; t0 < in_chunk; t0 += CAM_TILE) {
            const int nc = (int)(in_chunk - t0 < CAM_TILE ? in_chunk - t0 : CAM_TILE);
            hipLaunchKernelGGL(tex_shade, dim3(pb, (unsigned)nc), dim3(THREADS), 0, s, vertices, faces, n_v, n_f, a, texture, K, poses, c0 + t0,
                               c0 + t0, W, H, background[0], background[1], background[2],
                               (const unsigned long long*)(keys + (size_t)t0 * pixels), image, face_index, depth);
        }
    }
    return launched();
}
