// libngp_meshchart.so: a texture atlas made of charts, and a renderer of the mesh textured that way (C ABI and the exact rule:
// ngp_meshchart.h beside this file).  Compiled with -ffp-contract=off: every f32 and f64 expression below is the header's,
// operation by operation.  Every decision is an integer one, so the numpy restatement agrees bit for bit.
//
//   chart_class      one thread per face: the snapped corners, the int64 normal, the class;
//   vf_count, vf_scan, vf_fill   the vertex -> faces table by count, scan (one workgroup, ../mesh_scan.h) and fill;
//   label_init, label_union, label_scan, label_assign   union-find over faces (the forty lines of meshfilter.hip, copied): a face
//                    walks the lists of its three vertices and unites with every smaller active face of its class that shares two
//                    indices; roots are minima, so the labels do not depend on the order; chart ids by a scan over the root flags;
//   chart_bounds_init, chart_bounds   atomic minima and maxima of the plane coordinates per chart;
//   chart_raster     one thread per face: a box of at most SMALL_TEXELS texel centres is walked by the face's lane, a larger one by
//                    the whole wave (as ../mesh_raster.h walks pixels); int64 edge functions, an unsigned atomic minimum;
//   chart_overlap, chart_clear, chart_count   the same walk, reading: a face that finds another owner is evicted; its texels go;
//   chart_dilate     one thread per texel, eight neighbours in the header's order, ping-pong;
//   chart_corners    one thread per face: atlas coordinates and six f64 expressions;
//   chart_points     one thread per texel of the caller's range;
//   chart_keys, chart_shade   the shared rasteriser with KeySink, and one thread per pixel.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ngp_meshchart.h"

namespace {

#include "../mesh_host.h"
#include "../mesh_scan.h"

constexpr int THREADS = 256;
constexpr int MAX_WH = 16384;
constexpr int NO_CLASS = NGP_MESHCHART_NO_CLASS;
constexpr int SMALL_TEXELS = 64;                        // texel centres a lane walks on its own
constexpr unsigned NO_OWNER = 0xFFFFFFFFu;
constexpr float INF = __builtin_inff();
constexpr unsigned long long NO_KEY = ~0ull;

inline bool finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

inline bool image_ok(int W, int H) { return W >= 1 && H >= 1 && W <= MAX_WH && H <= MAX_WH; }

inline bool texel_size_ok(float s) { return s > 0.f && isfinite(s); }

inline float snap_scale(float s) { return (float)(16.0 / (double)s); }

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

// ---- snap and class --------------------------------------------------------------------------------------------------------------

// the class of the face with corners idx (all in range), and its corners in sixteenths of a texel
__device__ inline int snap_class(const float* __restrict__ vertices, const int idx[3], float c, int X[3][3]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* p = vertices + 3 * (size_t)idx[k];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float t = p[a] * c;
            const bool fits = fabsf(t) < 4194304.0f;   // false for NaN and infinities
            ok = ok && fits;
            X[k][a] = fits ? (int)rintf(t) : 0;
        }
    }
    if (!ok) return NO_CLASS;
    long long d1[3], d2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        d1[a] = (long long)X[1][a] - X[0][a];
        d2[a] = (long long)X[2][a] - X[0][a];
    }
    const long long n[3] = {d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]};
    int k = 0;
    long long best = n[0] < 0 ? -n[0] : n[0];
#pragma unroll
    for (int a = 1; a < 3; ++a) {
        const long long m = n[a] < 0 ? -n[a] : n[a];
        if (m > best) {
            best = m;
            k = a;
        }
    }
    if (best == 0) return NO_CLASS;
    return 2 * k + (n[k] < 0 ? 1 : 0);
}

// the plane coordinates of a snapped corner in the chart plane of class cls < 6
__device__ inline void plane_of(int cls, const int X[3], int& u, int& v) {
    const int k = cls >> 1;
    const int a = k == 2 ? 0 : k + 1, b = k == 0 ? 2 : k - 1;           // (k + 1) % 3, (k + 2) % 3
    const int xa = a == 0 ? X[0] : (a == 1 ? X[1] : X[2]), xb = b == 0 ? X[0] : (b == 1 ? X[1] : X[2]);
    u = (cls & 1) ? xb : xa;
    v = (cls & 1) ? xa : xb;
}

// a face of a chart in the atlas: its corners in sixteenths
struct Placed {
    long long x[3], y[3];
};

// face f's class and, when it has one and its chart lies in [lo, hi), its atlas corners; false otherwise
__device__ inline bool place_face(const float* __restrict__ vertices, const int* __restrict__ faces, long long f, unsigned n_v, float c,
                                  const int* __restrict__ face_chart, const int* __restrict__ chart_rects, long long lo, long long hi, int pad,
                                  Placed& pl, int idx[3]) {
    if (!load_face(faces, f, n_v, idx)) return false;
    const long long chart = face_chart[f];
    if (chart < lo || chart >= hi) return false;
    int X[3][3];
    const int cls = snap_class(vertices, idx, c, X);
    if (cls >= NO_CLASS) return false;
    const int* r = chart_rects + 6 * chart;
    const long long tx = 16 * ((long long)r[0] + pad - r[4]), ty = 16 * ((long long)r[1] + pad - r[5]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int u, v;
        plane_of(cls, X[k], u, v);
        pl.x[k] = tx + u;
        pl.y[k] = ty + v;
    }
    return true;
}

// the header's edge function of the edge p -> q at P, and its tie rule
__device__ inline long long edge_fn(long long px, long long py, long long qx, long long qy, long long Px, long long Py) {
    return (qx - px) * (Py - py) - (qy - py) * (Px - px);
}

__device__ inline bool edge_in(long long px, long long py, long long qx, long long qy, long long Px, long long Py) {
    const long long dx = qx - px, dy = qy - py;
    const long long E = dx * (Py - py) - dy * (Px - px);
    return E > 0 || (E == 0 && (dy > 0 || (dy == 0 && dx < 0)));
}

__device__ inline bool covers(const Placed& p, int i, int j) {
    const long long Px = 16ll * i + 8, Py = 16ll * j + 8;
    return edge_in(p.x[0], p.y[0], p.x[1], p.y[1], Px, Py) && edge_in(p.x[1], p.y[1], p.x[2], p.y[2], Px, Py) &&
           edge_in(p.x[2], p.y[2], p.x[0], p.y[0], Px, Py);
}

__global__ __launch_bounds__(THREADS) void chart_class(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                       long long n_f, float c, uint8_t* __restrict__ face_class) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_f) return;
    int idx[3], X[3][3];
    face_class[f] = (uint8_t)(load_face(faces, f, (unsigned)n_v, idx) ? snap_class(vertices, idx, c, X) : NO_CLASS);
}

// ---- the vertex -> faces table -----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void vf_count(const int* __restrict__ faces, long long n_v, long long n_f, int* count) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    int idx[3];
    if (f >= n_f || !load_face(faces, f, (unsigned)n_v, idx)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) atomicAdd(count + idx[k], 1);
}

// one workgroup: the exclusive scan of the counts, the total behind it, and the counts cleared to serve as cursors
__global__ __launch_bounds__(SCAN_THREADS) void vf_scan(int* __restrict__ count, long long n_v, long long* __restrict__ offsets) {
    __shared__ long long s[2][SCAN_THREADS];
    const long long total = scan_array([=](long long v) { return (long long)count[v]; }, n_v, offsets, s);
    if (threadIdx.x == 0) offsets[n_v] = total;
    for (long long v = threadIdx.x; v < n_v; v += SCAN_THREADS) count[v] = 0;
}

__global__ __launch_bounds__(THREADS) void vf_fill(const int* __restrict__ faces, long long n_v, long long n_f,
                                                   const long long* __restrict__ offsets, int* cursor, int* __restrict__ vf_faces) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    int idx[3];
    if (f >= n_f || !load_face(faces, f, (unsigned)n_v, idx)) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long pos = offsets[idx[k]] + atomicAdd(cursor + idx[k], 1);
        if (pos >= 0 && pos < 3 * n_f) vf_faces[pos] = (int)f;
    }
}

// ---- labels: union-find over faces ---------------------------------------------------------------------------------------------------

__device__ inline int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x by path halving; parent[x] only ever moves to a smaller ancestor (atomicMin), whichever thread gets there first
__device__ inline int find_root(int* parent, int x) {
    for (;;) {
        const int p = ld(parent + x);
        if (p == x) return x;
        const int g = ld(parent + p);
        if (g == p) return p;
        atomicMin(parent + x, g);
        x = g;
    }
}

__device__ inline void unite(int* parent, int a, int b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;                                        // hi was hooked elsewhere meanwhile: go on from its new parent
        b = lo;
    }
}

__global__ __launch_bounds__(THREADS) void label_init(long long n_f, int* __restrict__ parent) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (f < n_f) parent[f] = (int)f;
}

__device__ inline bool is_active(const uint8_t* __restrict__ face_class, const uint8_t* __restrict__ active, long long f) {
    return active[f] != 0 && face_class[f] < NO_CLASS;
}

__global__ __launch_bounds__(THREADS) void label_union(const int* __restrict__ faces, long long n_v, long long n_f,
                                                       const uint8_t* __restrict__ face_class, const uint8_t* __restrict__ active,
                                                       const long long* __restrict__ vf_offsets, const int* __restrict__ vf_faces,
                                                       int* parent) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    int idx[3];
    if (f >= n_f || !is_active(face_class, active, f) || !load_face(faces, f, (unsigned)n_v, idx)) return;
    const int cls = face_class[f];
    for (int k = 0; k < 3; ++k) {
        long long e0 = vf_offsets[idx[k]], e1 = vf_offsets[idx[k] + 1];
        if (e0 < 0) e0 = 0;
        if (e1 > 3 * n_f) e1 = 3 * n_f;
        for (long long e = e0; e < e1; ++e) {
            const int g = vf_faces[e];
            int gi[3];
            if (g < 0 || g >= f || !is_active(face_class, active, g) || face_class[g] != cls) continue;
            if (!load_face(faces, g, (unsigned)n_v, gi)) continue;
            int common = 0;
#pragma unroll
            for (int a = 0; a < 3; ++a) common += (gi[a] == idx[0] || gi[a] == idx[1] || gi[a] == idx[2]) ? 1 : 0;
            if (common >= 2) unite(parent, (int)f, g);
        }
    }
}

// one workgroup: the exclusive scan of the root flags of the active faces, and the number of charts
__global__ __launch_bounds__(SCAN_THREADS) void label_scan(const int* __restrict__ parent, const uint8_t* __restrict__ face_class,
                                                           const uint8_t* __restrict__ active, long long n_f,
                                                           long long* __restrict__ offsets, long long* __restrict__ n_charts) {
    __shared__ long long s[2][SCAN_THREADS];
    const long long total = scan_array(
        [=](long long f) { return (long long)((is_active(face_class, active, f) && parent[f] == (int)f) ? 1 : 0); }, n_f, offsets, s);
    if (threadIdx.x == 0) *n_charts = total;
}

__global__ __launch_bounds__(THREADS) void label_assign(int* parent, const uint8_t* __restrict__ face_class,
                                                        const uint8_t* __restrict__ active, long long n_f,
                                                        const long long* __restrict__ offsets, long long chart_base,
                                                        int* __restrict__ face_label, int* __restrict__ face_chart) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_f) return;
    if (!is_active(face_class, active, f)) {
        face_label[f] = -1;
        return;
    }
    const int r = find_root(parent, (int)f);
    face_label[f] = r;
    face_chart[f] = (int)(chart_base + offsets[r]);
}

// ---- bounds ------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void chart_bounds_init(long long n, int* __restrict__ bounds) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i < 4 * n) bounds[i] = (i & 3) < 2 ? INT32_MAX : INT32_MIN;
}

__global__ __launch_bounds__(THREADS) void chart_bounds(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                        long long n_f, float c, const int* __restrict__ face_chart, long long lo,
                                                        long long hi, int* bounds) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    int idx[3], X[3][3];
    if (f >= n_f || !load_face(faces, f, (unsigned)n_v, idx)) return;
    const long long chart = face_chart[f];
    if (chart < lo || chart >= hi) return;
    const int cls = snap_class(vertices, idx, c, X);
    if (cls >= NO_CLASS) return;
    int u0 = INT32_MAX, v0 = INT32_MAX, u1 = INT32_MIN, v1 = INT32_MIN;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int u, v;
        plane_of(cls, X[k], u, v);
        u0 = min(u0, u);
        v0 = min(v0, v);
        u1 = max(u1, u);
        v1 = max(v1, v);
    }
    int* b = bounds + 4 * (chart - lo);
    if (u0 < ld(b)) atomicMin(b, u0);
    if (v0 < ld(b + 1)) atomicMin(b + 1, v0);
    if (u1 > ld(b + 2)) atomicMax(b + 2, u1);
    if (v1 > ld(b + 3)) atomicMax(b + 3, v1);
}

// ---- ownership ---------------------------------------------------------------------------------------------------------------------

// what a lane hands to the wave: its face's atlas corners, the clipped box of texels and the face
struct Job {
    Placed p;
    int i0, i1, j0, j1;
    unsigned face;
};

struct OwnSink {                                        // the owner: the smallest covering face
    unsigned* owner;
    __device__ void operator()(size_t texel, unsigned face) const {
        if (face < __hip_atomic_load(owner + texel, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(owner + texel, face);
    }
};

struct OverlapSink {                                    // a covered centre that another face owns evicts the face
    const unsigned* owner;
    uint8_t* evicted;
    __device__ void operator()(size_t texel, unsigned face) const {
        if (owner[texel] != face) evicted[face] = 1;
    }
};

// The body of chart_raster and chart_overlap: one thread per face; sink(texel, face) for every texel centre inside the atlas that
// the face covers.  The loops after the ballot are wave-uniform.
template <class Sink>
__device__ __forceinline__ void walk_faces(const Sink& sink, const float* __restrict__ vertices, const int* __restrict__ faces,
                                           long long n_v, long long n_f, float c, const int* __restrict__ face_chart,
                                           const int* __restrict__ chart_rects, long long lo, long long hi, int pad, int W, int H) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    Job t;
    int idx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) t.p.x[k] = t.p.y[k] = 0;
    bool ok = f < n_f && place_face(vertices, faces, f, (unsigned)n_v, c, face_chart, chart_rects, lo, hi, pad, t.p, idx);
    t.face = (unsigned)f;
    long long x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    if (ok) {                                           // centres 16 i + 8 inside [min, max]: i from (min + 7) >> 4 to (max - 8) >> 4
        x0 = (min(min(t.p.x[0], t.p.x[1]), t.p.x[2]) + 7) >> 4;
        x1 = (max(max(t.p.x[0], t.p.x[1]), t.p.x[2]) - 8) >> 4;
        y0 = (min(min(t.p.y[0], t.p.y[1]), t.p.y[2]) + 7) >> 4;
        y1 = (max(max(t.p.y[0], t.p.y[1]), t.p.y[2]) - 8) >> 4;
        x0 = max(x0, 0ll);
        y0 = max(y0, 0ll);
        x1 = min(x1, (long long)W - 1);
        y1 = min(y1, (long long)H - 1);
        ok = x0 <= x1 && y0 <= y1;
    }
    t.i0 = ok ? (int)x0 : 0;                            // inside [0, W - 1] x [0, H - 1] when ok
    t.i1 = ok ? (int)x1 : -1;
    t.j0 = ok ? (int)y0 : 0;
    t.j1 = ok ? (int)y1 : -1;
    const bool big = ok && (t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1) > SMALL_TEXELS;   // at most 2^28
    if (ok && !big) {
        for (int j = t.j0; j <= t.j1; ++j)
            for (int i = t.i0; i <= t.i1; ++i)
                if (covers(t.p, i, j)) sink((size_t)j * W + i, t.face);
    }
    unsigned long long todo = __ballot(big);
    while (todo) {                                      // the wave walks each large box together
        const int leader = __ffsll((long long)todo) - 1;
        Job w;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            w.p.x[k] = __shfl(t.p.x[k], leader, 64);
            w.p.y[k] = __shfl(t.p.y[k], leader, 64);
        }
        w.i0 = __shfl(t.i0, leader, 64);
        w.i1 = __shfl(t.i1, leader, 64);
        w.j0 = __shfl(t.j0, leader, 64);
        w.j1 = __shfl(t.j1, leader, 64);
        w.face = (unsigned)__shfl((int)t.face, leader, 64);
        for (int j = w.j0 + (lane >> 3); j <= w.j1; j += 8)          // no cross-lane operation inside: lanes may run out apart
            for (int i = w.i0 + (lane & 7); i <= w.i1; i += 8)
                if (covers(w.p, i, j)) sink((size_t)j * W + i, w.face);
        todo &= todo - 1;
    }
}

__global__ __launch_bounds__(THREADS) void chart_raster(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                        long long n_f, float c, const int* __restrict__ face_chart,
                                                        const int* __restrict__ chart_rects, long long lo, long long hi, int pad, int W,
                                                        int H, unsigned* owner) {
    walk_faces(OwnSink{owner}, vertices, faces, n_v, n_f, c, face_chart, chart_rects, lo, hi, pad, W, H);
}

__global__ __launch_bounds__(THREADS) void chart_overlap(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                         long long n_f, float c, const int* __restrict__ face_chart,
                                                         const int* __restrict__ chart_rects, long long lo, long long hi, int pad, int W,
                                                         int H, const unsigned* owner, uint8_t* evicted) {
    walk_faces(OverlapSink{owner, evicted}, vertices, faces, n_v, n_f, c, face_chart, chart_rects, lo, hi, pad, W, H);
}

__global__ __launch_bounds__(THREADS) void chart_clear(unsigned* __restrict__ owner, long long texels, const uint8_t* __restrict__ evicted,
                                                       long long n_f) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= texels) return;
    const unsigned o = owner[t];
    if (o < (unsigned long long)n_f && evicted[o]) owner[t] = NO_OWNER;
}

__global__ __launch_bounds__(THREADS) void chart_count(const uint8_t* __restrict__ evicted, long long n_f, unsigned long long* n_evicted) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    const unsigned long long b = __ballot(f < n_f && evicted[f] != 0);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(n_evicted, (unsigned long long)__popcll(b));
}

__global__ __launch_bounds__(THREADS) void chart_dilate(const unsigned* __restrict__ src, unsigned* __restrict__ dst, int W, int H) {
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= (long long)W * H) return;
    const int y = (int)(t / W), x = (int)(t - (long long)y * W);
    unsigned o = src[t];
    if (o == NO_OWNER) {
        const int dx[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, dy[8] = {0, 0, -1, 1, -1, -1, 1, 1};
#pragma unroll
        for (int k = 7; k >= 0; --k) {                  // backwards, so that the first owned neighbour of the order is kept
            const int nx = x + dx[k], ny = y + dy[k];
            if (nx < 0 || ny < 0 || nx >= W || ny >= H) continue;
            const unsigned q = src[(size_t)ny * W + nx];
            if (q != NO_OWNER) o = q;
        }
    }
    dst[t] = o;
}

// ---- corners, UVs, texel points ------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void chart_corners(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                         long long n_f, float c, const int* __restrict__ face_chart,
                                                         const int* __restrict__ chart_rects, long long n_charts, int pad, int W, int H,
                                                         int* __restrict__ corner_texels, float* __restrict__ uvs) {
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (f >= n_f) return;
    Placed p;
    int idx[3];
    const bool ok = place_face(vertices, faces, f, (unsigned)n_v, c, face_chart, chart_rects, 0, n_charts, pad, p, idx);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int x = ok ? (int)p.x[k] : 0, y = ok ? (int)p.y[k] : 0;
        corner_texels[6 * (size_t)f + 2 * k] = x;
        corner_texels[6 * (size_t)f + 2 * k + 1] = y;
        uvs[6 * (size_t)f + 2 * k] = (float)(((double)x / 16.0) / (double)W);
        uvs[6 * (size_t)f + 2 * k + 1] = (float)(1.0 - ((double)y / 16.0) / (double)H);
    }
}

__global__ __launch_bounds__(THREADS) void chart_points(const float* __restrict__ vertices, const int* __restrict__ faces,
                                                        const float* __restrict__ normals, long long n_v, long long n_f,
                                                        const int* __restrict__ corner_texels, int W,
                                                        const int* __restrict__ texel_face, Box box, long long begin, long long count,
                                                        float* __restrict__ points, float* __restrict__ dirs,
                                                        uint8_t* __restrict__ valid) {
    const long long k = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (k >= count) return;
    const long long g = begin + k;
    const int row = (int)(g / W), col = (int)(g - (long long)row * W);
    float p[3] = {box.lo[0], box.lo[1], box.lo[2]}, d[3] = {0.f, 0.f, 1.f};
    bool ok = false;
    const int f = texel_face[g];
    Placed pl;
    int idx[3];
    long long area = 0;
    if (f >= 0 && f < n_f && load_face(faces, f, (unsigned)n_v, idx)) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            pl.x[q] = corner_texels[6 * (size_t)f + 2 * q];
            pl.y[q] = corner_texels[6 * (size_t)f + 2 * q + 1];
        }
        area = edge_fn(pl.x[0], pl.y[0], pl.x[1], pl.y[1], pl.x[2], pl.y[2]);   // > 0 for a face with a chart; products below 2^63
    }
    if (area > 0) {
        const long long Px = 16ll * col + 8, Py = 16ll * row + 8;
        const long long eca = edge_fn(pl.x[2], pl.y[2], pl.x[0], pl.y[0], Px, Py), eab = edge_fn(pl.x[0], pl.y[0], pl.x[1], pl.y[1], Px, Py);
        const float u = (float)((double)eca / (double)area), v = (float)((double)eab / (double)area);
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
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        points[3 * (size_t)k + a] = p[a];
        dirs[3 * (size_t)k + a] = d[a];
    }
    valid[k] = ok ? 1 : 0;
}

// ---- render ------------------------------------------------------------------------------------------------------------------------

#include "../mesh_camera.h"
#include "../mesh_raster.h"

__global__ __launch_bounds__(THREADS) void chart_keys(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                      long long n_f, const float* __restrict__ K, const float* __restrict__ poses,
                                                      long long cam0, int nc, int W, int H, float near_distance, unsigned long long* keys) {
    raster_faces(KeySink{}, vertices, faces, n_v, n_f, K, poses, cam0, nc, W, H, near_distance, keys);
}

// grid: (blocks over H * W, cameras of the launch)
__global__ __launch_bounds__(THREADS) void chart_shade(const float* __restrict__ vertices, const int* __restrict__ faces, long long n_v,
                                                       long long n_f, const int* __restrict__ corner_texels,
                                                       const uint8_t* __restrict__ texture, int AW, int AH, const float* __restrict__ K,
                                                       const float* __restrict__ poses, long long cam0, int W, int H, float bg0, float bg1,
                                                       float bg2, const unsigned long long* __restrict__ keys, float* __restrict__ image,
                                                       int* __restrict__ face_index, float* __restrict__ depth) {
    const int pix = blockIdx.x * THREADS + threadIdx.x;   // W * H <= 2^28
    if (pix >= W * H) return;
    const int ci = blockIdx.y;
    const size_t in_px = (size_t)ci * H * W + pix, out_px = (size_t)(cam0 + ci) * H * W + pix;
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
        const int* ct = corner_texels + 6 * (size_t)kf;
        const float ax = (float)ct[0] / 16.0f, ay = (float)ct[1] / 16.0f, bx = (float)ct[2] / 16.0f, by = (float)ct[3] / 16.0f;
        const float cx = (float)ct[4] / 16.0f, cy = (float)ct[5] / 16.0f;
        const float X = ((ax + beta * (bx - ax)) + gamma * (cx - ax)) - 0.5f;
        const float Y = ((ay + beta * (by - ay)) + gamma * (cy - ay)) - 0.5f;
        atlas_bilinear(texture, AW, AH, X, Y, rgb);     // whatever corner_texels holds, every read stays inside the atlas
    }
    image[3 * out_px] = rgb[0];
    image[3 * out_px + 1] = rgb[1];
    image[3 * out_px + 2] = rgb[2];
    if (face_index) face_index[out_px] = face;
    if (depth) depth[out_px] = z;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------

inline unsigned grid_of(long long n) { return (unsigned)blocks_of(n, THREADS); }

// the arguments every placed-face entry point shares; 0, NGP_EINVAL or NGP_ERANGE
inline int check_placed(const float* vertices, const int32_t* faces, int64_t n_v, int64_t n_f, float s, const int32_t* face_chart,
                        const int32_t* chart_rects, int64_t n_charts, int pad, int W, int H) {
    if (n_v < 0 || n_f < 1 || n_charts < 1 || !image_ok(W, H) || pad < 0 || pad > NGP_MESHCHART_MAX_PAD) return NGP_EINVAL;
    if (n_v > INT32_MAX || n_f > INT32_MAX || n_charts > INT32_MAX) return NGP_ERANGE;
    if (!texel_size_ok(s)) return NGP_EINVAL;
    if (!faces || !face_chart || !chart_rects || (n_v > 0 && !vertices)) return NGP_EINVAL;
    return 0;
}

// the header's shelves at width W from y0: the height so far, origins written when not NULL
inline long long shelves(const int32_t* sizes, const int32_t* order, int64_t n, long long W, long long y0, int32_t* origins) {
    long long x = 0, y = y0, shelf = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int64_t i = order[r];
        const long long w = sizes[2 * i], h = sizes[2 * i + 1];
        if (x + w > W) {
            y += shelf;
            x = 0;
            shelf = 0;
        }
        if (origins) {
            origins[2 * i] = (int32_t)x;
            origins[2 * i + 1] = (int32_t)(y > INT32_MAX ? INT32_MAX : y);
        }
        x += w;
        if (h > shelf) shelf = h;
    }
    return y + shelf;
}

// order[lo..hi) sorted by the header's rule: a heap sort, in place, without an allocation
inline bool before(const int32_t* sizes, int32_t a, int32_t b) {
    if (sizes[2 * a + 1] != sizes[2 * b + 1]) return sizes[2 * a + 1] > sizes[2 * b + 1];
    if (sizes[2 * a] != sizes[2 * b]) return sizes[2 * a] > sizes[2 * b];
    return a < b;
}

inline void sift(const int32_t* sizes, int32_t* order, int64_t root, int64_t n) {
    for (;;) {
        int64_t child = 2 * root + 1;
        if (child >= n) return;
        if (child + 1 < n && before(sizes, order[child], order[child + 1])) ++child;   // the later of the two
        if (!before(sizes, order[root], order[child])) return;
        const int32_t t = order[root];
        order[root] = order[child];
        order[child] = t;
        root = child;
    }
}

inline void sort_order(const int32_t* sizes, int32_t* order, int64_t n) {
    for (int64_t i = n / 2 - 1; i >= 0; --i) sift(sizes, order, i, n);
    for (int64_t end = n - 1; end > 0; --end) {         // the latest of the rest moves to the end
        const int32_t t = order[0];
        order[0] = order[end];
        order[end] = t;
        sift(sizes, order, 0, end);
    }
}

}  // namespace

NGP_API int ngp_meshchart_abi_version(void) { return 1; }

NGP_API const char* ngp_meshchart_build_arch(void) { return "gfx950"; }

NGP_API size_t ngp_meshchart_classify_workspace_bytes(int64_t n_vertices, int64_t n_faces) {
    if (n_vertices < 0 || n_vertices > INT32_MAX || n_faces < 1 || n_faces > INT32_MAX) return 0;
    return align256((size_t)(n_vertices + 1) * 4);
}

NGP_API int ngp_meshchart_classify(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float texel_size,
                                   uint8_t* face_class, int64_t* vf_offsets, int32_t* vf_faces, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (n_vertices < 0 || n_faces < 1) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (!texel_size_ok(texel_size)) return NGP_EINVAL;
    if (!faces || !face_class || !vf_offsets || !vf_faces || !workspace || (n_vertices > 0 && !vertices)) return NGP_EINVAL;
    if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)vf_offsets & 7) != 0) return NGP_EINVAL;
    if (workspace_bytes < ngp_meshchart_classify_workspace_bytes(n_vertices, n_faces)) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long n_v = n_vertices, n_f = n_faces;
    int* count = (int*)workspace;
    hipLaunchKernelGGL(chart_class, dim3(grid_of(n_f)), dim3(THREADS), 0, s, vertices, faces, n_v, n_f, snap_scale(texel_size), face_class);
    hipError_t e = hipMemsetAsync(count, 0, (size_t)(n_v + 1) * 4, s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(vf_faces, 0xFF, (size_t)n_f * 12, s);            // -1: no face, should a slot stay unfilled
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(vf_count, dim3(grid_of(n_f)), dim3(THREADS), 0, s, faces, n_v, n_f, count);
    hipLaunchKernelGGL(vf_scan, dim3(1), dim3(SCAN_THREADS), 0, s, count, n_v, (long long*)vf_offsets);
    hipLaunchKernelGGL(vf_fill, dim3(grid_of(n_f)), dim3(THREADS), 0, s, faces, n_v, n_f, (const long long*)vf_offsets, count, vf_faces);
    return launched();
}

NGP_API size_t ngp_meshchart_label_workspace_bytes(int64_t n_faces) {
    if (n_faces < 1 || n_faces > INT32_MAX) return 0;
    return align256((size_t)n_faces * 8) + align256((size_t)n_faces * 4);
}

NGP_API int ngp_meshchart_label(const int32_t* faces, int64_t n_vertices, int64_t n_faces, const uint8_t* face_class, const uint8_t* active,
                                const int64_t* vf_offsets, const int32_t* vf_faces, int unite_faces, int64_t chart_base, int32_t* face_label,
                                int32_t* face_chart, int64_t* n_charts, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_vertices < 0 || n_faces < 1 || chart_base < 0) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX || chart_base > INT32_MAX - n_faces) return NGP_ERANGE;
    if (!faces || !face_class || !active || !vf_offsets || !vf_faces || !face_label || !face_chart || !n_charts || !workspace) return NGP_EINVAL;
    if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)n_charts & 7) != 0 || ((uintptr_t)vf_offsets & 7) != 0) return NGP_EINVAL;
    if (workspace_bytes < ngp_meshchart_label_workspace_bytes(n_faces)) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long n_v = n_vertices, n_f = n_faces;
    long long* offsets = (long long*)workspace;
    int* parent = (int*)((char*)workspace + align256((size_t)n_f * 8));
    hipLaunchKernelGGL(label_init, dim3(grid_of(n_f)), dim3(THREADS), 0, s, n_f, parent);
    if (unite_faces)
        hipLaunchKernelGGL(label_union, dim3(grid_of(n_f)), dim3(THREADS), 0, s, faces, n_v, n_f, face_class, active,
                           (const long long*)vf_offsets, vf_faces, parent);
    hipLaunchKernelGGL(label_scan, dim3(1), dim3(SCAN_THREADS), 0, s, (const int*)parent, face_class, active, n_f, offsets,
                       (long long*)n_charts);
    hipLaunchKernelGGL(label_assign, dim3(grid_of(n_f)), dim3(THREADS), 0, s, parent, face_class, active, n_f, (const long long*)offsets,
                       (long long)chart_base, face_label, face_chart);
    return launched();
}

NGP_API int ngp_meshchart_bounds(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float texel_size,
                                 const int32_t* face_chart, int64_t chart_lo, int64_t chart_hi, int32_t* chart_bounds_out, void* stream) {
    if (n_vertices < 0 || n_faces < 1 || chart_lo < 0 || chart_hi <= chart_lo) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX || chart_hi > INT32_MAX) return NGP_ERANGE;
    if (!texel_size_ok(texel_size)) return NGP_EINVAL;
    if (!faces || !face_chart || !chart_bounds_out || (n_vertices > 0 && !vertices)) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long n = chart_hi - chart_lo;
    hipLaunchKernelGGL(chart_bounds_init, dim3(grid_of(4 * n)), dim3(THREADS), 0, s, n, chart_bounds_out);
    hipLaunchKernelGGL(chart_bounds, dim3(grid_of(n_faces)), dim3(THREADS), 0, s, vertices, faces, (long long)n_vertices, (long long)n_faces,
                       snap_scale(texel_size), face_chart, (long long)chart_lo, (long long)chart_hi, chart_bounds_out);
    return launched();
}

NGP_API int ngp_meshchart_pack(const int32_t* sizes, int64_t n, int sorted, int width_in, int y0, int32_t* origins, int32_t* order, int* width,
                               int* height) {
    if (!sizes || !origins || !order || !width || !height || n < 1) return NGP_EINVAL;
    if (n > INT32_MAX) return NGP_ERANGE;
    if (width_in < 0 || width_in > MAX_WH || y0 < 0 || y0 > MAX_WH || (width_in == 0 && y0 != 0)) return NGP_EINVAL;
    long long widest = 0, area = 0;
    for (int64_t i = 0; i < n; ++i) {
        const long long w = sizes[2 * i], h = sizes[2 * i + 1];
        if (w < 1 || h < 1 || w > MAX_WH || h > MAX_WH) return NGP_EINVAL;
        if (width_in > 0 && w > width_in) return NGP_EINVAL;
        if (w > widest) widest = w;
        area += w * h;
    }
    for (int64_t i = 0; i < n; ++i) order[i] = (int32_t)i;
    if (sorted) sort_order(sizes, order, n);
    long long W = width_in;
    if (width_in == 0) {
        long long r = (long long)sqrt((double)area);
        while (r * r < area) ++r;
        while (r > 0 && (r - 1) * (r - 1) >= area) --r;   // r = ceil(sqrt(area))
        W = widest > r ? widest : r;
        while (W <= MAX_WH && shelves(sizes, order, n, W, 0, nullptr) > W) W += (W >> 4) > 1 ? (W >> 4) : 1;
        if (W > MAX_WH) return NGP_ERANGE;
    }
    const long long H = shelves(sizes, order, n, W, y0, nullptr);
    if (H > MAX_WH) return NGP_ERANGE;
    shelves(sizes, order, n, W, y0, origins);
    *width = (int)W;
    *height = (int)H;
    return 0;
}

NGP_API int ngp_meshchart_raster(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float texel_size,
                                 const int32_t* face_chart, const int32_t* chart_rects, int64_t n_charts, int64_t chart_lo, int64_t chart_hi,
                                 int pad, int width, int height, uint32_t* owner, void* stream) {
    const int rc = check_placed(vertices, faces, n_vertices, n_faces, texel_size, face_chart, chart_rects, n_charts, pad, width, height);
    if (rc) return rc;
    if (chart_lo < 0 || chart_lo > chart_hi || chart_hi > n_charts || !owner) return NGP_EINVAL;
    hipLaunchKernelGGL(chart_raster, dim3(grid_of(n_faces)), dim3(THREADS), 0, (hipStream_t)stream, vertices, faces, (long long)n_vertices,
                       (long long)n_faces, snap_scale(texel_size), face_chart, chart_rects, (long long)chart_lo, (long long)chart_hi, pad, width,
                       height, (unsigned*)owner);
    return launched();
}

NGP_API int ngp_meshchart_evict(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float texel_size,
                                const int32_t* face_chart, const int32_t* chart_rects, int64_t n_charts, int64_t chart_lo, int64_t chart_hi,
                                int pad, int width, int height, uint32_t* owner, uint8_t* evicted, int64_t* n_evicted, void* stream) {
    const int rc = check_placed(vertices, faces, n_vertices, n_faces, texel_size, face_chart, chart_rects, n_charts, pad, width, height);
    if (rc) return rc;
    if (chart_lo < 0 || chart_lo > chart_hi || chart_hi > n_charts || !owner || !evicted || !n_evicted) return NGP_EINVAL;
    if (((uintptr_t)n_evicted & 7) != 0) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long n_f = n_faces, texels = (long long)width * height;
    hipError_t e = hipMemsetAsync(evicted, 0, (size_t)n_f, s);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(n_evicted, 0, 8, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(chart_overlap, dim3(grid_of(n_f)), dim3(THREADS), 0, s, vertices, faces, (long long)n_vertices, n_f,
                       snap_scale(texel_size), face_chart, chart_rects, (long long)chart_lo, (long long)chart_hi, pad, width, height,
                       (const unsigned*)owner, evicted);
    hipLaunchKernelGGL(chart_clear, dim3(grid_of(texels)), dim3(THREADS), 0, s, (unsigned*)owner, texels, (const uint8_t*)evicted, n_f);
    hipLaunchKernelGGL(chart_count, dim3(grid_of(n_f)), dim3(THREADS), 0, s, (const uint8_t*)evicted, n_f, (unsigned long long*)n_evicted);
    return launched();
}

NGP_API int ngp_meshchart_dilate(uint32_t* owner, uint32_t* scratch, int width, int height, int pad, void* stream) {
    if (!image_ok(width, height) || pad < 0 || pad > NGP_MESHCHART_MAX_PAD || !owner || !scratch || owner == scratch) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long texels = (long long)width * height;
    unsigned *src = (unsigned*)owner, *dst = (unsigned*)scratch;
    for (int p = 0; p < pad; ++p) {
        hipLaunchKernelGGL(chart_dilate, dim3(grid_of(texels)), dim3(THREADS), 0, s, (const unsigned*)src, dst, width, height);
        unsigned* t = src;
        src = dst;
        dst = t;
    }
    if (src != (unsigned*)owner) {
        const hipError_t e = hipMemcpyAsync(owner, src, (size_t)texels * 4, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return (int)e;
    }
    return launched();
}

NGP_API int ngp_meshchart_corners(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces, float texel_size,
                                  const int32_t* face_chart, const int32_t* chart_rects, int64_t n_charts, int pad, int width, int height,
                                  int32_t* corner_texels, float* uvs, void* stream) {
    const int rc = check_placed(vertices, faces, n_vertices, n_faces, texel_size, face_chart, chart_rects, n_charts, pad, width, height);
    if (rc) return rc;
    if (!corner_texels || !uvs) return NGP_EINVAL;
    hipLaunchKernelGGL(chart_corners, dim3(grid_of(n_faces)), dim3(THREADS), 0, (hipStream_t)stream, vertices, faces, (long long)n_vertices,
                       (long long)n_faces, snap_scale(texel_size), face_chart, chart_rects, (long long)n_charts, pad, width, height,
                       corner_texels, uvs);
    return launched();
}

NGP_API int ngp_meshchart_texel_points(const float* vertices, const int32_t* faces, const float* normals, int64_t n_vertices, int64_t n_faces,
                                       const int32_t* corner_texels, int width, int height, const int32_t* texel_face, const float* box,
                                       int64_t begin, int64_t count, float* points, float* dirs, uint8_t* valid, void* stream) {
    if (begin < 0 || count < 0 || !image_ok(width, height)) return NGP_EINVAL;
    const long long total = (long long)width * height;
    if (!box || begin > total || count > total - begin) return NGP_EINVAL;
    if (!finite3(box) || !finite3(box + 3) || !(box[0] <= box[3] && box[1] <= box[4] && box[2] <= box[5])) return NGP_EINVAL;
    if (n_vertices < 0 || n_faces < 1) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    if (count == 0) return 0;                           // nothing to write: the outputs may be empty
    if (!faces || !corner_texels || !texel_face || !points || !dirs || !valid || (n_vertices > 0 && (!vertices || !normals)))
        return NGP_EINVAL;
    Box b;
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = box[k];
        b.hi[k] = box[3 + k];
    }
    hipLaunchKernelGGL(chart_points, dim3(grid_of(count)), dim3(THREADS), 0, (hipStream_t)stream, vertices, faces, normals,
                       (long long)n_vertices, (long long)n_faces, corner_texels, width, texel_face, b, (long long)begin, (long long)count,
                       points, dirs, valid);
    return launched();
}

NGP_API size_t ngp_meshchart_render_workspace_bytes(int W, int H, int64_t n_cams) {
    if (!image_ok(W, H) || n_cams < 1 || n_cams > INT32_MAX) return 0;
    return (size_t)8 * W * H * (size_t)n_cams;
}

NGP_API int ngp_meshchart_render(const float* vertices, const int32_t* faces, int64_t n_vertices, int64_t n_faces,
                                 const int32_t* corner_texels, const uint8_t* texture, int atlas_width, int atlas_height, const float* K,
                                 const float* poses, int64_t n_cams, int W, int H, float near_distance, const float* background,
                                 void* workspace, size_t workspace_bytes, float* image, int32_t* face_index, float* depth, void* stream) {
    if (n_vertices < 0 || n_faces < 1 || n_cams < 1 || !image_ok(W, H) || !image_ok(atlas_width, atlas_height)) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX || n_cams > INT32_MAX) return NGP_ERANGE;
    if (!faces || !corner_texels || !texture || !K || !poses || !background || !workspace || !image || (n_vertices > 0 && !vertices))
        return NGP_EINVAL;
    if (((uintptr_t)workspace & 7) != 0) return NGP_EINVAL;
    if (!isfinite(near_distance) || !finite3(background)) return NGP_EINVAL;
    const size_t pixels = (size_t)W * H;
    const size_t fit = workspace_bytes / (8 * pixels);
    if (fit < 1) return NGP_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long n_v = n_vertices, n_f = n_faces;
    const unsigned fb = grid_of(n_f), pb = grid_of((long long)pixels);
    unsigned long long* keys = (unsigned long long*)workspace;
    const long long chunk = (long long)(fit < (size_t)n_cams ? fit : (size_t)n_cams);
    for (long long c0 = 0; c0 < n_cams; c0 += chunk) {
        const long long in_chunk = n_cams - c0 < chunk ? n_cams - c0 : chunk;
        const hipError_t e = hipMemsetAsync(keys, 0xFF, (size_t)in_chunk * pixels * 8, s);
        if (e != hipSuccess) return (int)e;
        for (long long t0 = 0; t0 < in_chunk; t0 += CAM_TILE) {
            const int nc = (int)(in_chunk - t0 < CAM_TILE ? in_chunk - t0 : CAM_TILE);
            hipLaunchKernelGGL(chart_keys, dim3(fb), dim3(THREADS), 0, s, vertices, faces, n_v, n_f, K, poses, c0 + t0, nc, W, H,
                               near_distance, keys + (size_t)t0 * pixels);
        }
        for (long long t0 = 0; t0 < in_chunk; t0 += CAM_TILE) {
            const int nc = (int)(in_chunk - t0 < CAM_TILE ? in_chunk - t0 : CAM_TILE);
            hipLaunchKernelGGL(chart_shade, dim3(pb, (unsigned)nc), dim3(THREADS), 0, s, vertices, faces, n_v, n_f, corner_texels, texture,
                               atlas_width, atlas_height, K, poses, c0 + t0, W, H, background[0], background[1], background[2],
                               (const unsigned long long*)(keys + (size_t)t0 * pixels), image, face_index, depth);
        }
    }
    return launched();
}
