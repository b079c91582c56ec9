// The triangle rasteriser of the mesh stages, shared by libngp_meshcull.so, libngp_meshtex.so and libngp_meshatlas.so, so that the
// cull's depth buffer, the textured renders and, through the cull, the photo bake see the same surface bit for bit.  Each library
// includes this header inside its own anonymous namespace and compiles with -ffp-contract=off.  The includer supplies, before it:
//   mesh_camera.h;
//   constexpr int THREADS, the workgroup size of its raster and shade kernels;
//   __device__ bool load_face(const int* faces, long long f, unsigned n_v, int idx[3]): reads face f, false if an index is
//   outside [0, n_v);
// and wraps raster_faces in a kernel of its own with the sink of its buffer:
//     struct Sink { using Word = ...; __device__ void operator()(Word* buf, size_t pixel, float z, unsigned face) const; };
// buf holds W * H words per camera of the launch, cleared by the includer to a word no sink value exceeds; a sink reads the pixel
// and takes an atomic minimum, so a word only ever falls and which walker or lane visits a pixel changes the time only.
#ifndef NGP_MESH_RASTER_H
#define NGP_MESH_RASTER_H

constexpr int CAM_TILE = 128;                           // cameras per launch: 12 floats each in LDS
constexpr int SMALL_BOX = 64;                           // pixels a lane walks on its own

// a face on one camera's screen: the points A, B, C, 1 / d of each, the signed area, the clipped pixel box and the face's index
struct Tri {
    float ax, ay, bx, by, cx, cy, qa, qb, qc, area;
    int i0, i1, j0, j1;
    unsigned face;
};

__device__ inline float edge(float ax, float ay, float bx, float by, float px, float py) { return (bx - ax) * (py - ay) - (by - ay) * (px - ax); }

__device__ inline void load_corners(const float* __restrict__ vertices, const int idx[3], float x[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* p = vertices + 3 * (size_t)idx[k];
        x[k][0] = p[0];
        x[k][1] = p[1];
        x[k][2] = p[2];
    }
}

// the three vertices x of a face in the camera o: screen points, q and area into t, the three depths out
__device__ inline void project_face(const float* o, const Intrinsics& in, const float x[3][3], Tri& t, float& da, float& db, float& dc) {
    project(o, in, x[0][0], x[0][1], x[0][2], t.ax, t.ay, da);
    project(o, in, x[1][0], x[1][1], x[1][2], t.bx, t.by, db);
    project(o, in, x[2][0], x[2][1], x[2][2], t.cx, t.cy, dc);
    t.qa = 1.0f / da;
    t.qb = 1.0f / db;
    t.qc = 1.0f / dc;
    t.area = edge(t.ax, t.ay, t.bx, t.by, t.cx, t.cy);
}

// the cull's buffer: the minimum of the depth's bits; the face is not kept
struct DepthSink {
    using Word = unsigned;
    __device__ void operator()(Word* buf, size_t pixel, float z, unsigned) const {
        Word* p = buf + pixel;
        const unsigned bits = __float_as_uint(z);
        if (bits < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, bits);
    }
};

// the renderers' buffer: the minimum of (depth bits, face), so that the smaller face index wins a tie in depth
struct KeySink {
    using Word = unsigned long long;
    __device__ void operator()(Word* buf, size_t pixel, float z, unsigned face) const {
        Word* p = buf + pixel;
        const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | face;
        if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
    }
};

// pixel (i, j), inside [0, W) x [0, H), of the camera whose words are buf: inside test on the centre, perspective-correct depth
template <class Sink>
__device__ inline void visit(const Sink& sink, const Tri& t, int i, int j, typename Sink::Word* buf, int W) {
    const float px = (float)i + 0.5f, py = (float)j + 0.5f;
    const float wa = edge(t.bx, t.by, t.cx, t.cy, px, py), wb = edge(t.cx, t.cy, t.ax, t.ay, px, py), wc = edge(t.ax, t.ay, t.bx, t.by, px, py);
    const bool covered = t.area > 0.f ? (wa >= 0.f && wb >= 0.f && wc >= 0.f) : (wa <= 0.f && wb <= 0.f && wc <= 0.f);
    if (!covered) return;
    const float z = t.area / (wa * t.qa + wb * t.qb + wc * t.qc);
    if (!(z > 0.f && z < __builtin_inff())) return;
    sink(buf, (size_t)j * W + i, z, t.face);
}

// The body of a raster kernel of THREADS threads: one work item per (face, camera).  A thread holds its face's three vertices in
// registers and walks the nc <= CAM_TILE cameras of the launch from cam0 on (their rows in LDS), re-projecting the vertices for
// each.  A clipped pixel box of at most SMALL_BOX pixels is walked by the face's own lane; larger boxes are collected with a ballot
// and walked by the whole wave, one box after the other, the lanes as an 8 x 8 pixel tile that strides the box.  Forced inline: the
// body is then optimised inside its kernel, as when it was written there, not on its own first.
template <class Sink>
__device__ __forceinline__ void raster_faces(const Sink& sink, const float* __restrict__ vertices, const int* __restrict__ faces,
                                             long long n_v, long long n_f, const float* __restrict__ K, const float* __restrict__ poses,
                                             long long cam0, int nc, int W, int H, float near_distance, typename Sink::Word* buf) {
    __shared__ float s_cam[12 * CAM_TILE];
    for (int i = threadIdx.x; i < nc; i += blockDim.x) camera_rows(poses + 12 * (size_t)(cam0 + i), s_cam + 12 * i);
    __syncthreads();
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    int idx[3];
    const bool valid = f < n_f && load_face(faces, f, (unsigned)n_v, idx);
    float x[3][3] = {};
    if (valid) load_corners(vertices, idx, x);
    const Intrinsics in = load_intrinsics(K);
    const int lane = threadIdx.x & 63;
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);
    for (int ci = 0; ci < nc; ++ci) {                   // wave-uniform: every lane takes part in the ballots below
        const float* o = s_cam + 12 * ci;
        typename Sink::Word* cb = buf + (size_t)ci * H * W;
        Tri t;
        float da, db, dc;
        project_face(o, in, x, t, da, db, dc);
        t.face = (unsigned)f;
        bool ok = valid && da >= near_distance && db >= near_distance && dc >= near_distance;
        ok = ok && t.area != 0.f && fabsf(t.area) < __builtin_inff();
        const float fi0 = fmaxf(0.f, floorf(fminf(fminf(t.ax, t.bx), t.cx))), fi1 = fminf(wmax, floorf(fmaxf(fmaxf(t.ax, t.bx), t.cx)));
        const float fj0 = fmaxf(0.f, floorf(fminf(fminf(t.ay, t.by), t.cy))), fj1 = fminf(hmax, floorf(fmaxf(fmaxf(t.ay, t.by), t.cy)));
        ok = ok && fi0 <= fi1 && fj0 <= fj1;            // false when a bound is NaN
        t.i0 = ok ? (int)fi0 : 0;                       // inside [0, W - 1] x [0, H - 1] when ok
        t.i1 = ok ? (int)fi1 : -1;
        t.j0 = ok ? (int)fj0 : 0;
        t.j1 = ok ? (int)fj1 : -1;
        // the box's area in int: W and H are at most 16384, so each factor lies in [0, 2^14] and the product is at most 2^28
        const bool big = ok && (t.i1 - t.i0 + 1) * (t.j1 - t.j0 + 1) > SMALL_BOX;
        if (ok && !big) {
            for (int j = t.j0; j <= t.j1; ++j)
                for (int i = t.i0; i <= t.i1; ++i) visit(sink, t, i, j, cb, W);
        }
        unsigned long long todo = __ballot(big);        // the same mask in every lane: the loop below is wave-uniform
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
            w.face = (unsigned)__shfl((int)t.face, leader, 64);
            for (int j = w.j0 + (lane >> 3); j <= w.j1; j += 8)      // no cross-lane operation inside: lanes may run out apart
                for (int i = w.i0 + (lane & 7); i <= w.i1; i += 8) visit(sink, w, i, j, cb, W);
            todo &= todo - 1;
        }
    }
}

// ---- what the two shade kernels share: one thread per pixel whose key names a face the raster accepted

// the winning face, corners idx, re-projected in the camera of pose P as the raster projected it: the perspective-correct
// weights of B and C at the centre of pixel pix of an image W wide, clamped to [0, 1]
__device__ inline void winner_weights(const float* __restrict__ vertices, const int idx[3], const float* __restrict__ K,
                                      const float* __restrict__ P, int pix, int W, float& beta, float& gamma) {
    float o[12], x[3][3];
    camera_rows(P, o);
    load_corners(vertices, idx, x);
    const Intrinsics in = load_intrinsics(K);
    Tri t;
    float da, db, dc;
    project_face(o, in, x, t, da, db, dc);
    const int j = pix / W, i = pix - j * W;
    const float px = (float)i + 0.5f, py = (float)j + 0.5f;
    const float wa = edge(t.bx, t.by, t.cx, t.cy, px, py), wb = edge(t.cx, t.cy, t.ax, t.ay, px, py), wc = edge(t.ax, t.ay, t.bx, t.by, px, py);
    const float la = wa * t.qa, lb = wb * t.qb, lc = wc * t.qc;
    const float sum = (la + lb) + lc;
    beta = fminf(fmaxf(lb / sum, 0.f), 1.f);
    gamma = fminf(fmaxf(lc / sum, 0.f), 1.f);
}

// the bilinear RGB, in [0, 1], at (X, Y) of an atlas AW x AH of 3 bytes per texel; the includers' X and Y are finite and below 2^17,
// so the casts are exact, and the clamps keep every read inside the atlas whatever X and Y are
__device__ inline void atlas_bilinear(const uint8_t* __restrict__ texture, int AW, int AH, float X, float Y, float rgb[3]) {
    const float flx = floorf(X), fly = floorf(Y);
    const float fx = X - flx, fy = Y - fly;
    const int i0 = min(max((int)flx, 0), AW - 1), j0 = min(max((int)fly, 0), AH - 1);
    const int i1 = min(i0 + 1, AW - 1), j1 = min(j0 + 1, AH - 1);
    const uint8_t *t00 = texture + 3 * ((size_t)j0 * AW + i0), *t10 = texture + 3 * ((size_t)j0 * AW + i1);
    const uint8_t *t01 = texture + 3 * ((size_t)j1 * AW + i0), *t11 = texture + 3 * ((size_t)j1 * AW + i1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = (float)t00[c] * (1.0f - fx) + (float)t10[c] * fx;
        const float bot = (float)t01[c] * (1.0f - fx) + (float)t11[c] * fx;
        rgb[c] = (top * (1.0f - fy) + bot * fy) / 255.0f;
    }
}

#endif
