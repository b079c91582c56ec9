// libngp_meshatlas.so: a texture atlas whose texel density follows the size of every face, and a renderer of the mesh textured that
// way (C ABI and the exact rule: ngp_meshatlas.h beside this file).  Compiled with -ffp-contract=off: every f32 expression below is the
// header's, operation by operation.  No ABI header or source of csrc/meshtex/ is compiled in: the two renderers share only the
// device code of ../mesh_camera.h and ../mesh_raster.h.
//
//   Classify, a stable counting sort of one digit with 16 buckets, blocks of BLOCK_FACES consecutive faces:
//   atlas_count    the class of every face (three squared edge lengths, at most 16 compares) and the block's histogram: one ballot
//                  per class and round, lane c of a wave keeps the count of class c, the waves meet in LDS;
//   atlas_scan     one workgroup: the exclusive int64 scan of blocks x classes, class-major from class 15 down, and the 16 totals;
//   atlas_scatter  a face's rank among the faces of its class in its wave from four ballots over the class's bits and a popcount
//                  under the lane mask; the waves' counts per round and class go to LDS, sixteen threads scan them in face order,
//                  and the position is block offset + wave offset + lane rank.  No atomic operation decides a position.
//   atlas_place    one thread per rank: class from base[], cell and slot, the record of its face.
//   atlas_points   one thread per texel of the caller's range: the band from y (the table of at most 16 bands is a kernel argument,
//                  walked by an unrolled select), row and column by one division each, slot, face through `order`, the three
//                  vertices and normals; consecutive texels of a row share one or two faces.
//   atlas_uvs      one thread per face: six f64 expressions.
//   Render, per chunk of as many cameras as the caller's workspace holds, on the caller's stream: the keys cleared to all ones,
//   atlas_raster   the shared rasteriser of ../mesh_raster.h with the sink KeySink: a 64-bit atomic minimum of (depth bits, face),
//                  skipped when the pixel already holds a smaller key;
//   atlas_shade    one thread per pixel: the winning face re-projected (../mesh_raster.h), its T, origin and slot from face_place,
//                  the bilinear lookup of ../mesh_raster.h with the four texels clamped into the atlas.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ngp_meshatlas.h"

namespace {

#include "../mesh_host.h"
#include "../mesh_scan.h"

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int ITERS = 8;
constexpr int BLOCK_FACES = THREADS * ITERS;            // 2048
constexpr int NC = NGP_MESHATLAS_CLASSES;
constexpr int MAX_WH = 16384;
constexpr float INF = __builtin_inff();
constexpr unsigned long long NO_KEY = ~0ull;

// T_c: 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256
__host__ __device__ inline int ladder(int c) { return c < 4 ? c + 1 : ((c & 1) ? 8 << ((c - 4) >> 1) : 3 << (((c - 4) >> 1) + 1)); }

inline bool finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

inline bool image_ok(int W, int H) { return W >= 1 && H >= 1 && W <= MAX_WH && H <= MAX_WH; }

// ---- the layout (host) ---------------------------------------------------------------------------------------------------------

struct Plan {
    int W, H, top;
    int y[NC], h[NC], cpr[NC], cells[NC];
    long long base[NC], count[NC], n;
};

inline long long height_at(const Plan& p, int W) {
    long long H = 0;
    for (int c = 0; c < NC; ++c) {
        if (!p.count[c]) continue;
        const long long cpr = W / (ladder(c) + 5), cells = (p.count[c] + 1) / 2;
        H += (cells + cpr - 1) / cpr * (ladder(c) + 4);
    }
    return H;
}

// the header's layout; 0, NGP_EINVAL or NGP_ERANGE
inline int plan_layout(const int64_t* counts, Plan& p) {
    if (!counts) return NGP_EINVAL;
    p.n = 0;
    p.top = -1;
    for (int c = 0; c < NC; ++c) {
        if (counts[c] < 0) return NGP_EINVAL;
        if (counts[c] > INT32_MAX) return NGP_ERANGE;
        p.count[c] = counts[c];
        p.n += counts[c];
        if (counts[c]) p.top = c;
    }
    if (p.n < 1) return NGP_EINVAL;
    if (p.n > INT32_MAX) return NGP_ERANGE;
    int lo = ladder(p.top) + 5, hi = MAX_WH;            // every non-empty class has cpr >= 1 from lo on
    if (height_at(p, hi) > hi) return NGP_ERANGE;
    while (lo < hi) {                                   // H(W) - W falls with W: the smallest W with H(W) <= W
        const int mid = (lo + hi) / 2;
        if (height_at(p, mid) <= mid) hi = mid;
        else lo = mid + 1;
    }
    p.W = lo;
    long long y = 0, base = 0;
    for (int c = NC - 1; c >= 0; --c) {
        p.base[c] = base;
        base += p.count[c];
        p.y[c] = p.h[c] = p.cpr[c] = p.cells[c] = 0;
        if (!p.count[c]) continue;
        p.cpr[c] = p.W / (ladder(c) + 5);
        p.cells[c] = (int)((p.count[c] + 1) / 2);
        p.h[c] = (int)((p.cells[c] + (long long)p.cpr[c] - 1) / p.cpr[c] * (ladder(c) + 4));
        p.y[c] = (int)y;
        y += p.h[c];
    }
    p.H = (int)y;
    return 0;
}

// what the kernels need of a Plan: small ints, passed by value
struct Bands {
    int y[NC], cpr[NC], cells[NC], base[NC], count[NC];
    int W, H;
};

inline Bands bands_of(const Plan& p) {
    Bands b;
    for (int c = 0; c < NC; ++c) {
        b.y[c] = p.y[c];
        b.cpr[c] = p.cpr[c];
        b.cells[c] = p.cells[c];
        b.base[c] = (int)p.base[c];
        b.count[c] = (int)p.count[c];
    }
    b.W = p.W;
    b.H = p.H;
    return b;
}

struct Box {
    float lo[3], hi[3];
};

// ---- classify ------------------------------------------------------------------------------------------------------------------

__device__ inline bool load_face(const int* __restrict__ faces, long long f, unsigned n_v, int idx[3]) {
    idx[0] = faces[3 * f];
    idx[1] = faces[3 * f + 1];
    idx[2] = faces[3 * f + 2];
    return (unsigned)idx[0] < n_v && (unsigned)idx[1] < n_v && (unsigned)idx[2] < n_v;
}

__device__ inline bool finite(float x) { return fabsf(x) < INF; }   // false for NaN

__device__ inline float edge2(const float* __restrict__ p, const float* __restrict__ q) {
    const float d0 = q[0] - p[0], d1 = q[1] - p[1], d2 = q[2] - p[2];
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

__device__ inline int class_of(const float* __restrict__ vertices, const int* __restrict__ faces, long long f, unsigned n_v, float s,
                               int cmin, int cmax) {
    int idx[3];
    if (!load_face(faces, f, n_v, idx)) return cmin;
    const float *A = vertices + 3 * (size_t)idx[0], *B = vertices + 3 * (size_t)idx[1], *C = vertices + 3 * (size_t)idx[2];
    const float eab = edge2(A, B), ebc = edge2(B, C), eca = edge2(C, A);
    float m = eab;
    if (ebc > m) m = ebc;
    if (eca > m) m = eca;
    if (!finite(m)) return cmin;
    int cls = cmax;
    for (int c = cmax; c >= cmin; --c) {                // t * t does not fall with c: the last hit is the smallest c
        const float t = (float)ladder(c) * s;
        if (m <= t * t) cls = c;
    }
    return cls;
}

// hist: class-major from class 15 down, hist[(15 - c) * nb + block]
__global__ __launch_bounds__(THREADS) void atlas_count(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                       long long n_f, float s, int cmin, int cmax, uint8_t* __restrict__ face_class,
                                                       int* __restrict__ hist, int nb) {
    __shared__ int s_h[WAVES][NC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * BLOCK_FACES;
    int mine = 0;                                       // lane c < 16: faces of class c this wave has seen
    for (int r = 0; r < ITERS; ++r) {                   // block-uniform: every lane takes part in the ballots
        const long long f = base + r * THREADS + threadIdx.x;
        int cls = -1;
        if (f < n_f) {
            cls = class_of(vertices, faces, f, (unsigned)n_v, s, cmin, cmax);
            face_class[f] = (uint8_t)cls;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const unsigned long long b = __ballot(cls == c);
            if (lane == c) mine += __popcll(b);
        }
    }
    if (lane < NC) s_h[w][lane] = mine;
    __syncthreads();
    if (threadIdx.x < NC) {
        int total = 0;
#pragma unroll
        for (int q = 0; q < WAVES; ++q) total += s_h[q][threadIdx.x];
        hist[(size_t)(NC - 1 - threadIdx.x) * nb + blockIdx.x] = total;
    }
}

// exclusive int64 scan of hist[0..n) into offsets by one workgroup, and the 16 class totals
__global__ __launch_bounds__(SCAN_THREADS) void atlas_scan(const int* __restrict__ hist, int nb, long long* __restrict__ offsets,
                                                           long long* __restrict__ counts) {
    __shared__ long long s[2][SCAN_THREADS];
    const int t = threadIdx.x;
    const long long total = scan_array([=](long long b) { return (long long)hist[b]; }, (long long)NC * nb, offsets, s);
    // scan_array closed with a barrier: class 15 - t begins at offsets[t * nb] and ends where the next one begins
    if (t < NC) counts[NC - 1 - t] = (t + 1 < NC ? offsets[(size_t)(t + 1) * nb] : total) - offsets[(size_t)t * nb];
}

__global__ __launch_bounds__(THREADS) void atlas_scatter(const uint8_t* __restrict__ face_class, long long n_f,
                                                         const long long* __restrict__ offsets, int nb, int* __restrict__ order) {
    __shared__ int s_wc[ITERS][WAVES][NC];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * BLOCK_FACES;
    for (int i = threadIdx.x; i < ITERS * WAVES * NC; i += THREADS) (&s_wc[0][0][0])[i] = 0;
    __syncthreads();
    int cls[ITERS], rank[ITERS];
    const unsigned long long below = (1ull << lane) - 1;
#pragma unroll
    for (int r = 0; r < ITERS; ++r) {                   // block-uniform: every lane takes part in the ballots
        const long long f = base + r * THREADS + threadIdx.x;
        const bool active = f < n_f;
        cls[r] = active ? (face_class[f] & (NC - 1)) : 0;
        unsigned long long m = __ballot(active);        // the lanes of my class: one ballot per bit of the class
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const bool bit = (cls[r] >> b) & 1;
            const unsigned long long bb = __ballot(active && bit);
            m &= bit ? bb : ~bb;
        }
        rank[r] = __popcll(m & below);
        if (active && rank[r] == 0) s_wc[r][w][cls[r]] = __popcll(m);
        if (!active) cls[r] = -1;
    }
    __syncthreads();
    if (threadIdx.x < NC) {                             // per class: exclusive scan over (round, wave), which is face order
        int run = 0;
        for (int r = 0; r < ITERS; ++r)
            for (int q = 0; q < WAVES; ++q) {
                const int v = s_wc[r][q][threadIdx.x];
                s_wc[r][q][threadIdx.x] = run;
                run += v;
            }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ITERS; ++r) {
        if (cls[r] < 0) continue;
        const long long pos = offsets[(size_t)(NC - 1 - cls[r]) * nb + blockIdx.x] + s_wc[r][w][cls[r]] + rank[r];
        if (pos >= 0 && pos < n_f) order[pos] = (int)(base + r * THREADS + threadIdx.x);
    }
}

__global__ __launch_bounds__(THREADS) void atlas_place(const int* __restrict__ order, long long n_f, Bands b, int* __restrict__ face_place) {
    const long long r = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (r >= n_f) return;
    int c = 0, base = 0, cpr = 1, y = 0;
#pragma unroll
    for (int k = 0; k < NC; ++k)
        if (b.count[k] > 0 && r >= b.base[k] && r < (long long)b.base[k] + b.count[k]) {
            c = k;
            base = b.base[k];
            cpr = b.cpr[k];
            y = b.y[k];
        }
    const int T = ladder(c);
    const int q = (int)r - base, g = q >> 1, slot = q & 1;
    const int gy = g / cpr, gx = g - gy * cpr;
    const int ox = gx * (T + 5), oy = y + gy * (T + 4);
    const int f = order[r];
    if ((unsigned)f >= (unsigned long long)n_f) return;
    face_place[2 * (size_t)f] = ox | (oy << 16);
    face_place[2 * (size_t)f + 1] = c | (slot << 8);
}

__global__ __launch_bounds__(THREADS) void atlas_points(const float* __restrict__ vertices, const int* __restrict__ faces,
                                                        const float* __restrict__ normals, long long n_v, long long n_f,
                                                        const int* __restrict__ order, Bands b, Box box, long long begin, long long count,
                                                        float* __restrict__ points, float* __restrict__ dirs, uint8_t* __restrict__ valid) {
    const long long k = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (k >= count) return;
    const int g = (int)(begin + k);                     // an atlas has at most 2^28 texels
    const int row = g / b.W, col = g - row * b.W;
    int c = -1, by = 0, cpr = 1, cells = 0, base = 0, cnt = 0;
#pragma unroll
    for (int q = NC - 1; q >= 0; --q)                   // the bands lie in this order: the last one that begins at or above the row
        if (b.count[q] > 0 && row >= b.y[q]) {
            c = q;
            by = b.y[q];
            cpr = b.cpr[q];
            cells = b.cells[q];
            base = b.base[q];
            cnt = b.count[q];
        }
    float p[3] = {box.lo[0], box.lo[1], box.lo[2]}, d[3] = {0.f, 0.f, 1.f};
    bool ok = false;
    if (c >= 0) {
        const int T = ladder(c), cw = T + 5, ch = T + 4;
        const int cy = (row - by) / ch, cx = col / cw;
        const int j = (row - by) - cy * ch, i = col - cx * cw;
        const long long cell = (long long)cy * cpr + cx;
        const bool slot1 = i + j > T + 3;
        const int is = slot1 ? T + 4 - i : i, js = slot1 ? T + 3 - j : j;
        const long long q = 2 * cell + (slot1 ? 1 : 0);
        int idx[3];
        if (cx < cpr && cell < cells && q < cnt) {
            const int f = order[base + q];
            if ((unsigned)f < (unsigned long long)n_f && load_face(faces, f, (unsigned)n_v, idx)) {
                const float u = (float)(is - 1) / (float)T, v = (float)(js - 1) / (float)T;
                const float *A = vertices + 3 * (size_t)idx[0], *B = vertices + 3 * (size_t)idx[1], *C = vertices + 3 * (size_t)idx[2];
                float x[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) x[a] = (A[a] + u * (B[a] - A[a])) + v * (C[a] - A[a]);
                ok = finite(x[0]) && finite(x[1]) && finite(x[2]);
                if (ok) {
                    const float *NA = normals + 3 * (size_t)idx[0], *NB = normals + 3 * (size_t)idx[1], *NCc = normals + 3 * (size_t)idx[2];
                    float n[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        p[a] = fminf(fmaxf(x[a], box.lo[a]), box.hi[a]);
                        n[a] = (NA[a] + u * (NB[a] - NA[a])) + v * (NCc[a] - NA[a]);
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
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        points[3 * (size_t)k + a] = p[a];
        dirs[3 * (size_t)k + a] = d[a];
    }
    valid[k] = ok ? 1 : 0;
}

// a face's record, by the header's masks
struct Place {
    int ox, oy, T, slot;
};

__device__ inline Place load_place(const int* __restrict__ face_place, size_t f) {
    const unsigned a = (unsigned)face_place[2 * f], b = (unsigned)face_place[2 * f + 1];
    Place pl;
    pl.ox = (int)(a & 0xFFFFu);
    pl.oy = (int)((a >> 16) & 0xFFFFu);
    pl.T = ladder((int)(b & 15u));
    pl.slot = (int)((b >> 8) & 1u);
    return pl;
}

__global__ __launch_bounds__(THREADS) void atlas_uvs(const int* __restrict__ face_place, long long n_f, int W, int H, float* __restrict__ uvs) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_f) return;
    const Place pl = load_place(face_place, (size_t)f);
    const int is[3] = {1, 1 + pl.T, 1}, js[3] = {1, 1, 1 + pl.T};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int gi = pl.ox + (pl.slot ? pl.T + 4 - is[k] : is[k]), gj = pl.oy + (pl.slot ? pl.T + 3 - js[k] : js[k]);
        uvs[6 * (size_t)f + 2 * k] = (float)(((double)gi + 0.5) / (double)W);
        uvs[6 * (size_t)f + 2 * k + 1] = (float)(1.0 - ((double)gj + 0.5) / (double)H);
    }
}

// ---- render --------------------------------------------------------------------------------------------------------------------

#include "../mesh_camera.h"
#include "../mesh_raster.h"

__global__ __launch_bounds__(THREADS) void atlas_raster(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                        long long n_f, const float* __restrict__ K, const float* __restrict__ poses,
                                                        long long cam0, int nc, int W, int H, float near_distance,
                                                        unsigned long long* keys) {
    raster_faces(KeySink{}, vertices, faces, n_v, n_f, K, poses, cam0, nc, W, H, near_distance, keys);
}

// grid: (blocks over H * W, cameras of the launch)
__global__ __launch_bounds__(THREADS) void atlas_shade(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                       long long n_f, const int* __restrict__ face_place, const uint8_t* __restrict__ texture,
                                                       int AW, int AH, const float* __restrict__ K, const float* __restrict__ poses,
                                                       long long cam0, long long out0, int W, int H, float bg0, float bg1, float bg2,
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
        const Place pl = load_place(face_place, (size_t)kf);
        const float xs = 1.0f + beta * (float)pl.T, ys = 1.0f + gamma * (float)pl.T;
        const float ox = (float)pl.ox, oy = (float)pl.oy;
        const float X = pl.slot ? ox + ((float)(pl.T + 4) - xs) : ox + xs;
        const float Y = pl.slot ? oy + ((float)(pl.T + 3) - ys) : oy + ys;
        atlas_bilinear(texture, AW, AH, X, Y, rgb);     // whatever face_place holds, every read stays inside the atlas
    }
    image[3 * out_px] = rgb[0];
    image[3 * out_px + 1] = rgb[1];
    image[3 * out_px + 2] = rgb[2];
    if (face_index) face_index[out_px] = face;
    if (depth) depth[out_px] = z;
}

struct ClassifyLayout {
    long long nb;
    size_t hist, offsets, total;
};

inline ClassifyLayout classify_layout(long long n_f) {
    ClassifyLayout l;
    l.nb = blocks_of(n_f, BLOCK_FACES);
    l.hist = 0;
    l.offsets = align256((size_t)NC * l.nb * 4);
    l.total = l.offsets + align256((size_t)NC * l.nb * 8);
    return l;
}

}  // namespace

NGP_API int ngp_meshatlas_abi_version(void) { return 1; }

NGP_API const char* ngp_meshatlas_build_arch(void) { return "gfx950"; }

NGP_API size_t ngp_meshatlas_classify_workspace_bytes(int64_t n_faces) {
    if (n_faces < 1 || n_faces > INT32_MAX) return 0;
    return classify_layout(n_faces).total;
}

NGP_API int ngp_meshatlas_classify(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float texel_size,
                                   int cmin, int cmax, uint8_t* face_class, int32_t* order, int64_t* counts, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    if (n_vertices < 0 || n_faces < 1) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (!(texel_size > 0.f) || !isfinite(texel_size)) return NGP_EINVAL;
    if (cmin < 0 || cmax >= NC || cmin > cmax) return NGP_EINVAL;
    if (!faces || !face_class || !order || !counts || !workspace || (n_vertices > 0 && !vertices)) return NGP_EINVAL;
    if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)counts & 7) != 0) return NGP_EINVAL;
    const ClassifyLayout l = classify_layout(n_faces);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    int* hist = (int*)(ws + l.hist);
    long long* offsets = (long long*)(ws + l.offsets);
    const int nb = (int)l.nb;
    hipLaunchKernelGGL(atlas_count, dim3((unsigned)nb), dim3(THREADS), 0, s, vertices, faces, (long long)n_vertices, (long long)n_faces,
                       texel_size, cmin, cmax, face_class, hist, nb);
    hipLaunchKernelGGL(atlas_scan, dim3(1), dim3(SCAN_THREADS), 0, s, (const int*)hist, nb, offsets, (long long*)counts);
    hipLaunchKernelGGL(atlas_scatter, dim3((unsigned)nb), dim3(THREADS), 0, s, (const uint8_t*)face_class, (long long)n_faces,
                       (const long long*)offsets, nb, order);
    return launched();
}

NGP_API int ngp_meshatlas_layout(const int64_t* counts, int* width, int* height, int32_t* bands) {
    if (!width || !height) return NGP_EINVAL;
    Plan p;
    const int rc = plan_layout(counts, p);
    if (rc) return rc;
    *width = p.W;
    *height = p.H;
    if (bands)
        for (int c = 0; c < NC; ++c) {
            bands[4 * c] = p.y[c];
            bands[4 * c + 1] = p.h[c];
            bands[4 * c + 2] = p.cpr[c];
            bands[4 * c + 3] = p.cells[c];
        }
    return 0;
}

NGP_API int ngp_meshatlas_place(const int32_t* order, const int64_t* counts, int64_t n_faces, int32_t* face_place, void* stream) {
    if (n_faces < 1) return NGP_EINVAL;
    Plan p;
    const int rc = plan_layout(counts, p);
    if (rc) return rc;
    if (p.n != n_faces || !order || !face_place) return NGP_EINVAL;
    hipLaunchKernelGGL(atlas_place, dim3((unsigned)blocks_of(n_faces, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, order,
                       (long long)n_faces, bands_of(p), face_place);
    return launched();
}

NGP_API int ngp_meshatlas_texel_points(const float* vertices, const int32_t* faces, const float* normals, int64_t n_vertices,
                                       int64_t n_faces, const int32_t* order, const int64_t* counts, const float* box, int64_t begin,
                                       int64_t count, float* points, float* dirs, uint8_t* valid, void* stream) {
    if (n_vertices < 0 || n_faces < 1 || begin < 0 || count < 0) return NGP_EINVAL;
    Plan p;
    const int rc = plan_layout(counts, p);
    if (rc) return rc;
    if (n_vertices > INT32_MAX) return NGP_ERANGE;
    if (p.n != n_faces) return NGP_EINVAL;
    const long long total = (long long)p.W * p.H;
    if (!box || begin > total || count > total - begin) return NGP_EINVAL;
    if (!finite3(box) || !finite3(box + 3) || !(box[0] <= box[3] && box[1] <= box[4] && box[2] <= box[5])) return NGP_EINVAL;
    if (count == 0) return 0;                           // nothing to write: the outputs may be empty
    if (!faces || !order || !points || !dirs || !valid || (n_vertices > 0 && (!vertices || !normals))) return NGP_EINVAL;
    Box b;
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = box[k];
        b.hi[k] = box[3 + k];
    }
    hipLaunchKernelGGL(atlas_points, dim3((unsigned)blocks_of(count, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, vertices, faces,
                       normals, (long long)n_vertices, (long long)n_faces, order, bands_of(p), b, (long long)begin, (long long)count, points,
                       dirs, valid);
    return launched();
}

NGP_API int ngp_meshatlas_face_uvs(const int32_t* face_place, int64_t n_faces, int width, int height, float* uvs, void* stream) {
    if (n_faces < 1 || !image_ok(width, height)) return NGP_EINVAL;
    if (n_faces > INT32_MAX) return NGP_ERANGE;
    if (!face_place || !uvs) return NGP_EINVAL;
    hipLaunchKernelGGL(atlas_uvs, dim3((unsigned)blocks_of(n_faces, THREADS)), dim3(THREADS), 0, (hipStream_t)stream, face_place,
                       (long long)n_faces, width, height, uvs);
    return launched();
}

NGP_API size_t ngp_meshatlas_render_workspace_bytes(int W, int H, int64_t n_cams) {
    if (!image_ok(W, H) || n_cams < 1 || n_cams > INT32_MAX) return 0;
    return (size_t)8 * W * H * (size_t)n_cams;
}

NGP_API int ngp_meshatlas_render(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces,
                                 const int32_t* face_place, const uint8_t* texture, int atlas_width, int atlas_height, const float* K,
                                 const float* poses, int64_t n_cams, int W, int H, float near_distance, const float* background,
                                 void* workspace, size_t workspace_bytes, float* image, int32_t* face_index, float* depth, void* stream) {
    if (n_vertices < 0 || n_faces < 1 || n_cams < 1 || !image_ok(W, H) || !image_ok(atlas_width, atlas_height)) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX || n_cams > INT32_MAX) return NGP_ERANGE;
    if (!faces || !face_place || !texture || !K || !poses || !background || !workspace || !image || (n_vertices > 0 && !vertices))
        return NGP_EINVAL;
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
            hipLaunchKernelGGL(atlas_raster, dim3(fb), dim3(THREADS), 0, s, vertices, faces, n_v, n_f, K, poses, c0 + t0, nc, W, H,
                               near_distance, keys + (size_t)t0 * pixels);
        }
        for (long long t0 = 0; t0 < in_chunk; t0 += CAM_TILE) {
            const int nc = (int)(in_chunk - t0 < CAM_TILE ? in_chunk - t0 : CAM_TILE);
            hipLaunchKernelGGL(atlas_shade, dim3(pb, (unsigned)nc), dim3(THREADS), 0, s, vertices, faces, n_v, n_f, face_place, texture,
                               atlas_width, atlas_height, K, poses, c0 + t0, c0 + t0, W, H, background[0], background[1], background[2],
                               (const unsigned long long*)(keys + (size_t)t0 * pixels), image, face_index, depth);
        }
    }
    return launched();
}
