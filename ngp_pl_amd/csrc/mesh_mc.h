// The per-point and per-cell rules of marching cubes (include/ngp_mesh.h), once: shared by libngp_mesh.so, which reads a dense
// volume, and libngp_meshsparse.so, which reads a brick's tile in LDS.  Included inside the including library's anonymous namespace
// after mesh/mc_tables.h, as mesh_scan.h is.  Every function is the plain f32 expression of the header, one rounding per operation
// (both libraries are compiled with -ffp-contract=off), so the two extractors give the same bits on the same sigma values.
#ifndef NGP_MESH_MC_H
#define NGP_MESH_MC_H

// coordinate of lattice point idx along one axis
__device__ __forceinline__ float mc_position(float lo, float h, int idx) { return lo + (float)idx * h; }

__device__ __forceinline__ int mc_inside(float sigma, float thr) { return sigma > thr; }

// where the surface cuts the edge from the owning endpoint a to b
__device__ __forceinline__ float mc_edge_t(float thr, float sa, float sb) {
    const float t = (thr - sa) / (sb - sa);
    return fminf(fmaxf(t, 0.0f), 1.0f);
}

// One component of the gradient at a point with index c of n along the axis: central, one-sided at the border.  at(d) is sigma at
// the point displaced by d = -1, 0, 1 along the axis; only displacements inside the lattice are asked for.
template <class At>
__device__ __forceinline__ float mc_grad_axis(At at, int c, int n, float h) {
    if (c == 0) return (at(1) - at(0)) / h;
    if (c == n - 1) return (at(0) - at(-1)) / h;
    return (at(1) - at(-1)) / (2.0f * h);
}

// The vertex on the edge along `axis` from a (position pa, gradient ga) to b (coordinate pb_axis along the axis, gradient gb):
// position, and the outward unit normal (0 for a zero gradient) when normal is not null.
__device__ __forceinline__ void mc_vertex(const float pa[3], int axis, float pb_axis, float t, const float ga[3], const float gb[3],
                                          float* __restrict__ position, float* __restrict__ normal) {
    float gv[3];
    for (int c = 0; c < 3; ++c) {
        const float pb = c == axis ? pb_axis : pa[c];
        position[c] = pa[c] + t * (pb - pa[c]);
        gv[c] = ga[c] + t * (gb[c] - ga[c]);
    }
    if (normal) {
        const float nrm = sqrtf(gv[0] * gv[0] + gv[1] * gv[1] + gv[2] * gv[2]);
        for (int c = 0; c < 3; ++c) normal[c] = nrm > 0.0f ? -gv[c] / nrm : 0.0f;
    }
}

// cube index of a cell from the inside bits of its corners, corner c at offset (c & 1, c >> 1 & 1, c >> 2 & 1)
template <class Inside>
__device__ __forceinline__ int mc_cube(Inside inside) {
    int cube = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) cube |= inside(c) << c;
    return cube;
}

// Corner k of triangle tr of a cube index: the edge's owning corner and its axis.  The vertex of that edge is number
// popc(crossed bits of the owner below the axis) past the owner's first vertex.
__device__ __forceinline__ void mc_face_corner(int cube, int tr, int k, int& corner, int& axis) {
    const int e = NGP_MC_TRIS[cube][3 * tr + k];
    corner = NGP_MC_EDGE_CORNERS[e][0];
    axis = e >> 2;
}

#endif
