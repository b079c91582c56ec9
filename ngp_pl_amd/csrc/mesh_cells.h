// The clustering grid of include/ngp_meshsimplify.h, once: libngp_meshquadric.so places a cluster's vertex correctly only if it
// bins vertices exactly as libngp_meshsimplify.so's clustering did.  Included inside the including library's anonymous namespace, as
// mesh_compact.h is, and compiled with -ffp-contract=off: the f32 expressions are the header's, operation by operation.
#ifndef NGP_MESH_CELLS_H
#define NGP_MESH_CELLS_H

constexpr float QF = 1048576.0f;                        // the header's Q
constexpr double QD = 1048576.0;
constexpr float CELLS = 2097152.0f;                     // 2^21 cells per axis

struct Grid {
    float o[3], cell;
};

__device__ inline Grid load_grid(const float* __restrict__ origin, float cell) { return Grid{{origin[0], origin[1], origin[2]}, cell}; }

// the header's "cell of a vertex": false when outside the grid
__device__ inline bool cell_of(const Grid& g, const float* __restrict__ x, int c[3], long long q[3]) {
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float t = (x[k] - g.o[k]) / g.cell;
        const float fl = floorf(t);
        const bool ok = fabsf(t) < __uint_as_float(0x7F800000u) && fl >= 0.f && fl < CELLS;    // false for NaN
        inside = inside && ok;
        c[k] = ok ? (int)fl : 0;
        q[k] = ok ? (long long)rintf((t - (float)c[k]) * QF) : 0;
    }
    return inside;
}

#endif
