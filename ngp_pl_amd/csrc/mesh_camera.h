// The pinhole camera of the mesh stages, shared by libngp_meshcull.so, libngp_meshtex.so, libngp_meshatlas.so, libngp_meshphoto.so
// and libngp_meshtsdf.so: each includes this header inside its own anonymous namespace, after <hip/hip_runtime.h>, and compiles
// with -ffp-contract=off, so that the f32 expressions below are the stage headers' m, s and projection, operation by operation.
// The includer supplies nothing else; where the rows go (LDS tile or registers), their stride and every barrier are the includer's.
#ifndef NGP_MESH_CAMERA_H
#define NGP_MESH_CAMERA_H

// the 9 entries of R^T, then -R^T t (the headers' m and s) of the row-major 3 x 4 pose P = [R | t], into o[0..12)
__device__ inline void camera_rows(const float* __restrict__ P, float* o) {
    const float t0 = P[3], t1 = P[7], t2 = P[11];
#pragma unroll
    for (int r = 0; r < 3; ++r) {                       // row r of R^T = column r of R
        const float a = P[r], b = P[4 + r], cc = P[8 + r];
        o[3 * r] = a;
        o[3 * r + 1] = b;
        o[3 * r + 2] = cc;
        o[9 + r] = -(a * t0 + b * t1 + cc * t2);
    }
}

struct Intrinsics {
    float k[9];
};

// the same for every thread: scalar loads
__device__ inline Intrinsics load_intrinsics(const float* __restrict__ K) {
    Intrinsics in;
#pragma unroll
    for (int i = 0; i < 9; ++i) in.k[i] = K[i];
    return in;
}

// the point (x, y, z) in the camera whose rows are o: pixel coordinates (u, v) and depth d, the divisions whatever d is
__device__ inline void project(const float* o, const Intrinsics& in, float x, float y, float z, float& u, float& v, float& d) {
    const float px = o[0] * x + o[1] * y + o[2] * z + o[9];
    const float py = o[3] * x + o[4] * y + o[5] * z + o[10];
    const float pz = o[6] * x + o[7] * y + o[8] * z + o[11];
    const float ud = in.k[0] * px + in.k[1] * py + in.k[2] * pz, vd = in.k[3] * px + in.k[4] * py + in.k[5] * pz;
    d = in.k[6] * px + in.k[7] * py + in.k[8] * pz;
    u = ud / d;
    v = vd / d;
}

#endif
