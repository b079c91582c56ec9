// libngp_metrics.so: the squared error behind PSNR and the structural similarity index with the 11-tap Gaussian window, per image
// of a batch (C ABI and the exact rule: include/ngp_metrics.h).  Compiled with -ffp-contract=off: every f32 expression below is
// the header's, operation by operation.
//
//   ssim_tile<C>  one workgroup of 256 threads per TILE_W x TILE_H = 64 x 12 windows of one image, all C channels, one launch for
//                 the batch.  (1) The (TILE_H + 10) x (TILE_W + 10) patch of pred and target goes into LDS with coalesced reads:
//                 in the channel-last layout a patch row is one run of C * 74 floats, in the planar layout C runs of 74; either
//                 way it is stored planar in LDS, [channel][row][x], so that the row pass reads consecutive words (a stride of C
//                 words would put lanes l and l + 32 / C on one bank).  Pixels outside the image are stored as 0 and feed only
//                 windows that are never counted or written.  (2) Per channel, the row pass forms the five filtered rows
//                 [map][row][x] in LDS, 22 x 64 work items over 256 threads, each 22 LDS reads.  (3) The column pass: thread
//                 (wave g, lane x) owns the windows of column x in rows 3g .. 3g + 2; per map it reads its column's 13 values
//                 (a wave reads 64 consecutive words per row: no bank conflict) and forms three sums, then the index, the map
//                 element and its own f64 sum.  (4) The wave's shuffle tree, the four waves in order, one partial per workgroup.
//                 LDS: 2 * C * 22 * 74 * 4 + 5 * 22 * 64 * 4 + 64 bytes = 41248, 54272, 67296, 80320 for C = 1 .. 4: three, three,
//                 two and two workgroups per CU of 160 KiB.
//   sq_tile       a grid-stride stream: at most SQ_MAX_BLOCKS workgroups per image, each striding the image's elements.
//   finish        one wave per image adds the image's partials (lane l the partials l, l + 64, ... in index order, then the tree).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../../include/ngp_metrics.h"

#define NGP_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int THREADS = 256;
constexpr int TW = NGP_METRICS_TILE_W, TH = NGP_METRICS_TILE_H;
constexpr int TAPS = NGP_METRICS_WINDOW_TAPS, HALO = TAPS - 1;
constexpr int PW = TW + HALO, PR = TH + HALO;              // the patch: 74 x 22
constexpr int ROWS_PER_WAVE = TH / (THREADS / 64);          // 3
constexpr int SQ_THREADS = NGP_METRICS_SQ_THREADS, SQ_MAX_BLOCKS = NGP_METRICS_SQ_MAX_BLOCKS;
static_assert(TW == 64 && TH % (THREADS / 64) == 0, "the column pass maps a wave onto one row of windows");

__device__ constexpr float G[TAPS] = NGP_METRICS_WINDOW;

// the fixed tree over a wave: lane 0 ends with ((l0 + l32) + (l16 + l48)) + ... of the 64 lanes
__device__ inline void wave_sum(double& s, long long& n) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off);
        n += __shfl_down(n, off);
    }
}

// lane 0 of every wave -> LDS, thread 0 adds the waves in index order and stores the workgroup's partial
template <int WAVES>
__device__ inline void block_store(double s, long long n, double* wave_s, long long* wave_n, double* out_s, long long* out_n, long long slot) {
    wave_sum(s, n);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) {
        wave_s[tid >> 6] = s;
        wave_n[tid >> 6] = n;
    }
    __syncthreads();
    if (tid == 0) {
        double a = wave_s[0];
        long long b = wave_n[0];
#pragma unroll
        for (int k = 1; k < WAVES; ++k) {
            a += wave_s[k];
            b += wave_n[k];
        }
        out_s[slot] = a;
        out_n[slot] = b;
    }
}

template <int C>
__global__ __launch_bounds__(THREADS) void ssim_tile(const float* __restrict__ pred, const float* __restrict__ target,
                                                      const uint8_t* __restrict__ mask, int tiles_x, int tiles_y, int h, int w, int layout,
                                                      float c1, float c2, double* __restrict__ part_s, long long* __restrict__ part_n,
                                                      float* __restrict__ map) {
    __shared__ float patch_p[C][PR][PW];
    __shared__ float patch_t[C][PR][PW];
    __shared__ float xf[5][PR][TW];
    __shared__ double wave_s[THREADS / 64];
    __shared__ long long wave_n[THREADS / 64];

    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    const int per_image = tiles_x * tiles_y;
    const long long img = b / per_image;
    const int tile = (int)(b - img * per_image);
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x0 = tx * TW, y0 = ty * TH;                   // the tile's first window = the patch's first pixel
    const int oh = h - HALO, ow = w - HALO;

    // (1) the patch
    for (int idx = tid; idx < C * PR * PW; idx += THREADS) {
        int ch, row, x;
        if (layout == NGP_METRICS_HWC) {
            row = idx / (PW * C);
            const int rem = idx - row * (PW * C);
            x = rem / C;
            ch = rem - x * C;
        } else {
            ch = idx / (PR * PW);
            const int rem = idx - ch * (PR * PW);
            row = rem / PW;
            x = rem - row * PW;
        }
        const int gy = y0 + row, gx = x0 + x;
        float p = 0.0f, t = 0.0f;
        if (gy < h && gx < w) {
            const long long at = layout == NGP_METRICS_HWC ? ((img * h + gy) * w + gx) * C + ch : ((img * C + ch) * h + gy) * w + gx;
            p = pred[at];
            t = target[at];
        }
        patch_p[ch][row][x] = p;
        patch_t[ch][row][x] = t;
    }

    // the thread's windows: column x0 + lane, rows y0 + 3 * wave ..
    const int lx = tid & 63, ly = (tid >> 6) * ROWS_PER_WAVE;
    const int ox = x0 + lx;
    bool inside[ROWS_PER_WAVE], selected[ROWS_PER_WAVE];
#pragma unroll
    for (int r = 0; r < ROWS_PER_WAVE; ++r) {
        const int oy = y0 + ly + r;
        inside[r] = oy < oh && ox < ow;
        selected[r] = inside[r] && (!mask || mask[(img * h + (oy + HALO / 2)) * w + (ox + HALO / 2)] != 0);
    }
    double sum = 0.0;
    long long count = 0;
    __syncthreads();

    for (int ch = 0; ch < C; ++ch) {
        // (2) the row pass of the five maps
        for (int idx = tid; idx < PR * TW; idx += THREADS) {
            const int row = idx >> 6, x = idx & 63;
            const float* pp_ = &patch_p[ch][row][x];
            const float* tp_ = &patch_t[ch][row][x];
            float p = pp_[0], t = tp_[0];
            float ap = G[0] * p, at = G[0] * t, app = G[0] * (p * p), att = G[0] * (t * t), apt = G[0] * (p * t);
#pragma unroll
            for (int k = 1; k < TAPS; ++k) {
                p = pp_[k];
                t = tp_[k];
                ap = ap + G[k] * p;
                at = at + G[k] * t;
                app = app + G[k] * (p * p);
                att = att + G[k] * (t * t);
                apt = apt + G[k] * (p * t);
            }
            xf[0][row][x] = ap;
            xf[1][row][x] = at;
            xf[2][row][x] = app;
            xf[3][row][x] = att;
            xf[4][row][x] = apt;
        }
        __syncthreads();

        // (3) the column pass and the index
        float f[5][ROWS_PER_WAVE];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            float v[ROWS_PER_WAVE + HALO];
#pragma unroll
            for (int j = 0; j < ROWS_PER_WAVE + HALO; ++j) v[j] = xf[m][ly + j][lx];
#pragma unroll
            for (int r = 0; r < ROWS_PER_WAVE; ++r) {
                float a = G[0] * v[r];
#pragma unroll
                for (int k = 1; k < TAPS; ++k) a = a + G[k] * v[r + k];
                f[m][r] = a;
            }
        }
#pragma unroll
        for (int r = 0; r < ROWS_PER_WAVE; ++r) {
            const float mp = f[0][r], mt = f[1][r], pp = f[2][r], tt = f[3][r], pt = f[4][r];
            const float spp = pp - mp * mp;
            const float stt = tt - mt * mt;
            const float spt = pt - mp * mt;
            const float num = ((2.0f * mp) * mt + c1) * (2.0f * spt + c2);
            const float den = ((mp * mp + mt * mt) + c1) * ((spp + stt) + c2);
            const float s = num / den;
            if (map && inside[r]) {
                const long long oy = y0 + ly + r;
                const long long at = layout == NGP_METRICS_HWC ? ((img * oh + oy) * ow + ox) * C + ch : ((img * C + ch) * oh + oy) * ow + ox;
                map[at] = s;
            }
            if (selected[r]) {
                sum += (double)s;
                count += 1;
            }
        }
        __syncthreads();                                    // the next channel's row pass overwrites xf
    }

    // (4) the workgroup's partial
    block_store<THREADS / 64>(sum, count, wave_s, wave_n, part_s, part_n, b);
}

__global__ __launch_bounds__(SQ_THREADS) void sq_tile(const float* __restrict__ pred, const float* __restrict__ target,
                                                       const uint8_t* __restrict__ mask, int blocks_per_image, long long pixels, int c, int layout,
                                                       double* __restrict__ part_s, long long* __restrict__ part_n) {
    __shared__ double wave_s[SQ_THREADS / 64];
    __shared__ long long wave_n[SQ_THREADS / 64];
    const long long b = blockIdx.x;
    const long long img = b / blocks_per_image;
    const long long blk = b - img * blocks_per_image;
    const long long elements = pixels * c, stride = (long long)blocks_per_image * SQ_THREADS;
    const float* p = pred + img * elements;
    const float* t = target + img * elements;
    const uint8_t* m = mask ? mask + img * pixels : nullptr;
    double sum = 0.0;
    long long count = 0;
    for (long long i = blk * SQ_THREADS + threadIdx.x; i < elements; i += stride) {
        if (m && m[layout == NGP_METRICS_HWC ? i / c : i % pixels] == 0) continue;
        const float d = p[i] - t[i];
        sum += (double)(d * d);
        count += 1;
    }
    block_store<SQ_THREADS / 64>(sum, count, wave_s, wave_n, part_s, part_n, b);
}

// one wave per image
__global__ __launch_bounds__(64) void finish(const double* __restrict__ part_s, const long long* __restrict__ part_n, int per_image,
                                             double* __restrict__ sum, long long* __restrict__ count) {
    const long long img = blockIdx.x;
    double s = 0.0;
    long long n = 0;
    for (int j = threadIdx.x; j < per_image; j += 64) {
        s += part_s[img * per_image + j];
        n += part_n[img * per_image + j];
    }
    wave_sum(s, n);
    if (threadIdx.x == 0) {
        sum[img] = s;
        count[img] = n;
    }
}

inline int launched() { return (int)hipGetLastError(); }

inline long long ssim_tiles(int h, int w) {                 // 0 where no window fits
    if (h <= HALO || w <= HALO) return 0;
    return (long long)((h - HALO + TH - 1) / TH) * ((w - HALO + TW - 1) / TW);
}

inline long long sq_blocks(int c, int h, int w) {
    const long long elements = (long long)c * h * w, blocks = (elements + SQ_THREADS - 1) / SQ_THREADS;
    return blocks < SQ_MAX_BLOCKS ? blocks : SQ_MAX_BLOCKS;
}

// the shared argument checks: 0, NGP_EINVAL or NGP_ERANGE
inline int check(const void* pred, const void* target, int64_t n, int c, int h, int w, int min_side, int layout, const void* workspace,
                 size_t workspace_bytes, const void* sum, const void* count) {
    if (!pred || !target || !workspace || !sum || !count) return NGP_EINVAL;
    if (n < 1 || c < 1 || c > NGP_METRICS_MAX_CHANNELS || h < min_side || w < min_side) return NGP_EINVAL;
    if (layout != NGP_METRICS_HWC && layout != NGP_METRICS_CHW) return NGP_EINVAL;
    if (h > NGP_METRICS_MAX_SIDE || w > NGP_METRICS_MAX_SIDE) return NGP_ERANGE;
    const size_t need = ngp_metrics_workspace_bytes(n, c, h, w);
    if (need == 0) return NGP_ERANGE;                       // more than INT32_MAX partials
    if (workspace_bytes < need || ((uintptr_t)workspace & 7) != 0) return NGP_EINVAL;
    return 0;
}

}  // namespace

NGP_API int ngp_metrics_abi_version(void) { return 1; }

NGP_API const char* ngp_metrics_build_arch(void) { return "gfx950"; }

NGP_API int ngp_metrics_tile(int* w, int* h) {
    if (!w || !h) return NGP_EINVAL;
    *w = TW;
    *h = TH;
    return 0;
}

NGP_API size_t ngp_metrics_workspace_bytes(int64_t n, int c, int h, int w) {
    if (n < 1 || c < 1 || c > NGP_METRICS_MAX_CHANNELS || h < 1 || w < 1 || h > NGP_METRICS_MAX_SIDE || w > NGP_METRICS_MAX_SIDE) return 0;
    const long long a = ssim_tiles(h, w), b = sq_blocks(c, h, w), per_image = a > b ? a : b;
    if (n > INT32_MAX / per_image) return 0;
    return (size_t)16 * (size_t)n * (size_t)per_image;
}

NGP_API int ngp_metrics_sq_error(const float* pred, const float* target, const uint8_t* mask, int64_t n, int c, int h, int w, int layout,
                                 void* workspace, size_t workspace_bytes, double* sum, int64_t* count, void* stream) {
    const int rc = check(pred, target, n, c, h, w, 1, layout, workspace, workspace_bytes, sum, count);
    if (rc) return rc;
    const int per_image = (int)sq_blocks(c, h, w);
    const long long total = (long long)n * per_image;
    double* part_s = (double*)workspace;
    long long* part_n = (long long*)(part_s + total);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sq_tile, dim3((unsigned)total), dim3(SQ_THREADS), 0, s, pred, target, mask, per_image, (long long)h * w, c, layout, part_s, part_n);
    hipLaunchKernelGGL(finish, dim3((unsigned)n), dim3(64), 0, s, (const double*)part_s, (const long long*)part_n, per_image, sum, (long long*)count);
    return launched();
}

NGP_API int ngp_metrics_ssim(const float* pred, const float* target, const uint8_t* mask, int64_t n, int c, int h, int w, int layout,
                             double data_range, void* workspace, size_t workspace_bytes, double* sum, int64_t* count, float* map,
                             void* stream) {
    const int rc = check(pred, target, n, c, h, w, TAPS, layout, workspace, workspace_bytes, sum, count);
    if (rc) return rc;
    if (!(data_range > 0.0) || !isfinite(data_range)) return NGP_EINVAL;
    const float c1 = (float)((0.01 * data_range) * (0.01 * data_range)), c2 = (float)((0.03 * data_range) * (0.03 * data_range));
    const int tiles_x = (w - HALO + TW - 1) / TW, tiles_y = (h - HALO + TH - 1) / TH, per_image = tiles_x * tiles_y;
    const long long total = (long long)n * per_image;
    double* part_s = (double*)workspace;
    long long* part_n = (long long*)(part_s + total);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)total), block(THREADS);
    switch (c) {
        case 1: hipLaunchKernelGGL(ssim_tile<1>, grid, block, 0, s, pred, target, mask, tiles_x, tiles_y, h, w, layout, c1, c2, part_s, part_n, map); break;
        case 2: hipLaunchKernelGGL(ssim_tile<2>, grid, block, 0, s, pred, target, mask, tiles_x, tiles_y, h, w, layout, c1, c2, part_s, part_n, map); break;
        case 3: hipLaunchKernelGGL(ssim_tile<3>, grid, block, 0, s, pred, target, mask, tiles_x, tiles_y, h, w, layout, c1, c2, part_s, part_n, map); break;
        default: hipLaunchKernelGGL(ssim_tile<4>, grid, block, 0, s, pred, target, mask, tiles_x, tiles_y, h, w, layout, c1, c2, part_s, part_n, map); break;
    }
    hipLaunchKernelGGL(finish, dim3((unsigned)n), dim3(64), 0, s, (const double*)part_s, (const long long*)part_n, per_image, sum, (long long*)count);
    return launched();
}
