// The nearest face of a mesh through a uniform grid of face lists, shared by libngp_meshdist.so (which also builds the grid) and
// libngp_meshnormal.so (which reads a grid that libngp_meshdist.so built), so that the two answers are one walk: with every
// candidate accepted, nearest_face returns the same key in both, bit for bit.  Each library includes this header inside its own
// anonymous namespace, after <hip/hip_runtime.h>, <math.h> and <stdint.h>, and compiles with -ffp-contract=off.  The includer
// supplies the constants of its own public header as arguments: the slack factor (SLACK of the stage headers) to nearest_face, the
// axis and cell limits to axes_ok and grid_magnitude; and to nearest_face the filter of its candidates,
//     struct Accept { __device__ bool operator()(V3 a, V3 b, V3 c) const; };  // a, b, c: the vertices of a usable face
#ifndef NGP_MESH_NEAREST_H
#define NGP_MESH_NEAREST_H

struct V3 {
    float x, y, z;
};
__device__ inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ inline V3 load3(const float* __restrict__ p, long long i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
__device__ inline bool finite3(V3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
__device__ inline float absmax3(V3 a) { return fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fabsf(a.z)); }

// the three vertices of a usable face; false otherwise
__device__ inline bool load_face(const float* __restrict__ v, const int32_t* __restrict__ f, int n_v, long long face, V3& a, V3& b, V3& c) {
    const int ia = f[3 * face], ib = f[3 * face + 1], ic = f[3 * face + 2];
    if ((unsigned)ia >= (unsigned)n_v || (unsigned)ib >= (unsigned)n_v || (unsigned)ic >= (unsigned)n_v) return false;
    a = load3(v, ia);
    b = load3(v, ib);
    c = load3(v, ic);
    return finite3(a) && finite3(b) && finite3(c);
}

// rule 2 of both stage headers: the closest point of (a, b, c) to p and the barycentric pair (of b and c) of the deciding case
__device__ inline V3 closest_point(V3 p, V3 a, V3 b, V3 c, float& bv, float& bw) {
    const V3 ab = sub(b, a), ac = sub(c, a), ap = sub(p, a);
    const float d1 = dot(ab, ap), d2 = dot(ac, ap);
    bv = 0.0f, bw = 0.0f;
    if (d1 <= 0.0f && d2 <= 0.0f) return a;
    const V3 bp = sub(p, b);
    const float d3 = dot(ab, bp), d4 = dot(ac, bp);
    if (d3 >= 0.0f && d4 <= d3) {
        bv = 1.0f;
        return b;
    }
    const float vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {
        const float v = d1 / (d1 - d3);
        bv = v;
        return {a.x + v * ab.x, a.y + v * ab.y, a.z + v * ab.z};
    }
    const V3 cp = sub(p, c);
    const float d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0f && d5 <= d6) {
        bw = 1.0f;
        return c;
    }
    const float vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {
        const float w = d2 / (d2 - d6);
        bw = w;
        return {a.x + w * ac.x, a.y + w * ac.y, a.z + w * ac.z};
    }
    const float va = d3 * d6 - d5 * d4;
    const float s43 = d4 - d3, s56 = d5 - d6;
    if (va <= 0.0f && s43 >= 0.0f && s56 >= 0.0f) {
        const float w = s43 / (s43 + s56);
        const V3 bc = sub(c, b);
        bv = 1.0f - w, bw = w;
        return {b.x + w * bc.x, b.y + w * bc.y, b.z + w * bc.z};
    }
    const float denom = 1.0f / ((va + vb) + vc);
    float v = vb * denom, w = vc * denom;
    if (!(v >= 0.0f)) v = 0.0f;
    if (v > 1.0f) v = 1.0f;
    if (!(w >= 0.0f)) w = 0.0f;
    const float rest = 1.0f - v;
    if (w > rest) w = rest;
    bv = v, bw = w;
    return {(a.x + v * ab.x) + w * ac.x, (a.y + v * ab.y) + w * ac.y, (a.z + v * ab.z) + w * ac.z};
}

__device__ inline V3 closest_point(V3 p, V3 a, V3 b, V3 c) {
    float bv, bw;
    return closest_point(p, a, b, c, bv, bw);
}

__device__ inline float squared_distance(V3 p, V3 q) {
    const V3 e = sub(p, q);
    return (e.x * e.x + e.y * e.y) + e.z * e.z;
}

// THE GRID: the clamped cell of a coordinate
__device__ inline int cell_of(float t, float o, float cell, int n) {
    const float g = floorf((t - o) / cell);
    if (!(g >= 0.0f)) return 0;
    if (g >= (float)n) return n - 1;
    return (int)g;
}

struct Grid {
    float ox, oy, oz, cell, m_grid;
    int nx, ny, nz;
};

// every candidate counts
struct AcceptAll {
    __device__ bool operator()(V3, V3, V3) const { return true; }
};

// The nearest face to the finite point p among the faces `accept` lets through, by shells of cells round p's cell: the key
// bits(d2) << 32 | face of the winner, the smaller face index on a tie, or ~0 when no shell within reach holds a candidate.  The
// best key lives in one 64-bit register pair; there is no per-thread array.  start[cell] .. start[cell + 1] is the cell's list in
// entries (n_entries in all).  The walk ends after the shell of radius r when the best distance plus the slack is within r cells,
// when r cells less the slack exceed max_dist, or when the next shell lies wholly outside the grid.  shells and evaluated, where
// given, count the shells walked and the faces whose distance was taken.  Forced inline: the walk is then optimised inside its
// kernel, as when it was written there, not on its own first.
template <class Accept>
__device__ __forceinline__ unsigned long long nearest_face(V3 p, const Accept& accept, const float* __restrict__ v,
                                                           const int32_t* __restrict__ f, int n_v, int n_f, Grid g, float slack_factor,
                                                           float max_dist, const uint32_t* __restrict__ start,
                                                           const int32_t* __restrict__ entries, int n_entries,
                                                           uint32_t* shells = nullptr, uint32_t* evaluated = nullptr) {
    unsigned long long best = ~0ull;
    uint32_t n_shells = 0, n_evaluated = 0;
    const float sq = slack_factor * fmaxf(g.m_grid, absmax3(p));
    const int cx = cell_of(p.x, g.ox, g.cell, g.nx), cy = cell_of(p.y, g.oy, g.cell, g.ny), cz = cell_of(p.z, g.oz, g.cell, g.nz);
    for (int r = 0;; ++r) {
        ++n_shells;
        const int z0 = max(cz - r, 0), z1 = min(cz + r, g.nz - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.ny - 1);
        for (int z = z0; z <= z1; ++z) {
            const bool zface = z == cz - r || z == cz + r;
            for (int y = y0; y <= y1; ++y) {
                // a row of the shell: all of [cx - r, cx + r] on a z or y face of the cube, else its two ends
                const bool full = zface || y == cy - r || y == cy + r;
                const int step = full || r == 0 ? 1 : 2 * r;
                for (int x = cx - r; x <= cx + r; x += step) {
                    if (x < 0 || x >= g.nx) continue;
                    const long long cell = ((long long)z * g.ny + y) * g.nx + x;
                    const uint32_t e0 = start[cell], e1 = min(start[cell + 1], (uint32_t)n_entries);
                    for (uint32_t e = e0; e < e1; ++e) {
                        const int face = entries[e];
                        if ((unsigned)face >= (unsigned)n_f) continue;
                        V3 a, b, c;
                        if (!load_face(v, f, n_v, face, a, b, c)) continue;
                        if (!accept(a, b, c)) continue;
                        const float d2 = squared_distance(p, closest_point(p, a, b, c));
                        ++n_evaluated;
                        if (!(d2 <= 3.402823466e38f)) continue;                 // not finite: contributes nothing
                        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)face;
                        best = key < best ? key : best;
                    }
                }
            }
        }
        const float rc = (float)r * g.cell;
        const float best_d2 = __uint_as_float((uint32_t)(best >> 32));          // NaN bits while nothing was found: the test is false
        if (sqrtf(best_d2) + sq <= rc) break;
        if (rc - sq > max_dist) break;
        const int q = r + 1;                                // the next shell lies wholly outside the grid
        if (cx - q < 0 && cx + q >= g.nx && cy - q < 0 && cy + q >= g.ny && cz - q < 0 && cz + q >= g.nz) break;
    }
    if (shells) *shells = n_shells;
    if (evaluated) *evaluated = n_evaluated;
    return best;
}

// ---- host side

inline bool axes_ok(int nx, int ny, int nz, int max_axis, long long max_cells) {
    return nx >= 1 && ny >= 1 && nz >= 1 && nx <= max_axis && ny <= max_axis && nz <= max_axis && (long long)nx * ny * nz <= max_cells;
}

// M_grid of the stage headers, or a negative value for a grid that is refused
inline float grid_magnitude(const float* origin, float cell, int nx, int ny, int nz, int max_axis, long long max_cells) {
    if (!origin || !axes_ok(nx, ny, nz, max_axis, max_cells) || !(cell > 0.0f) || !isfinite(cell)) return -1.0f;
    const int n[3] = {nx, ny, nz};
    float m = 0.0f;
    for (int k = 0; k < 3; ++k) {
        if (!isfinite(origin[k])) return -1.0f;
        const float far = origin[k] + (float)n[k] * cell;
        if (!isfinite(far)) return -1.0f;
        m = fmaxf(m, fmaxf(fabsf(origin[k]), fabsf(far)));
    }
    return m;
}

#endif
