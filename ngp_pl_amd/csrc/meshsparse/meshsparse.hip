// libngp_meshsparse.so: marching cubes over the 8^3-point bricks of the lattice that touch occupied cells (C ABI:
// ngp_meshsparse.h, beside this file).  The per-point and per-cell rules are ../mesh_mc.h, shared with libngp_mesh.so, so the two
// extractors give the same bits; sums and scans are ../mesh_scan.h.
//   sp_mask_small / sp_mask_box   occupancy bitfield -> mesh mask: one thread per brick where a grown brick spans at most two cells
//                       per axis, else one workgroup striding over the brick's cell box;
//   sp_dilate           sample mask = 26-neighbourhood dilation; per block of 2048 bricks the packed counts of both masks;
//   sp_scan_packed      one workgroup: exclusive int64 scans of both half-words of packed counts, the two totals to the caller: of
//                       the block counts here, of the sampled bricks' counts after sp_count;
//   sp_index_fill       scans within the block: brick table (brick -> sample slot, -1) and the two ascending brick lists;
//   sp_points           sample slots -> positions of their 512 points;
//   sp_count            one workgroup of 512 per SAMPLED brick, one thread per owned point and cell.  A vertex belongs to the result
//                       when its edge is crossed and one of the (up to four) cells round the edge lies in a meshed brick; those cells
//                       lie in the brick itself or in its neighbours at -1, so the owner decides alone, from eight mask bytes, and
//                       no brick writes another brick's flags.  A brick with no meshed brick among those eight owns no vertex and
//                       leaves before it reads the pool.  Writes the flag byte (bit 0 inside, bits 1-3 the +x/+y/+z vertices) and
//                       the brick's packed (triangles << 16 | vertices) count;
//   sp_emit_vertices    per sampled brick that owns a vertex: the 11^3 sigma tile (the brick and a halo of -1 .. +2) in LDS, a scan
//                       of the flags, positions, normals, keys and the points' int32 vertex offsets;
//   sp_emit_faces       per meshed brick: the 9^3 tile, cube indices, a scan of the triangle counts, the indices through the flags
//                       and vertex offsets of the owning points, which lie in the brick or its neighbours at +1.
// Neighbours are reached through the brick table; a neighbour outside the grid is absent and never read.  Workspace: 5 B per
// sampled point + 20 B per sampled brick.  Every order is fixed by brick number and local index and nothing is placed by an atomic:
// the output is bit-identical from run to run.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngp_meshsparse.h"

#define NGP_MC_STORAGE static __constant__ const
#include "../mesh/mc_tables.h"

namespace {

#include "../mesh_host.h"
#include "../mesh_scan.h"
#include "../mesh_mc.h"

constexpr int SB = NGP_MESHSPARSE_BRICK;
constexpr int SB3 = NGP_MESHSPARSE_BRICK_POINTS;
constexpr int SP_THREADS = SB3;                         // one thread per point of a brick
constexpr int IX_THREADS = 256;
constexpr int IX_ITERS = 8;
constexpr int IX_BLOCK = IX_THREADS * IX_ITERS;
constexpr int MAX_AXIS = 65535;
constexpr long long MAX_BRICKS = 1LL << 30;
static_assert(SB == 8 && SB3 == 512, "local indices are three 3-bit fields");
static_assert(3 * SB3 < (1 << 16) && NGP_MC_MAX_TRIS * SB3 < (1 << 15) && IX_BLOCK < (1 << 15), "packed counts overflow");

struct Dims {
    int nx, ny, nz;
    int nbx, nby, nbz;
    long long nb;
};

struct Geom {
    float lo[3], h[3];
};

struct Occ {
    double lo[3], h[3], margin, scale;
    int cascades, G;
};

__device__ inline void brick_xyz(long long b, const Dims& d, int& bx, int& by, int& bz) {
    const unsigned long long row = (unsigned long long)b / (unsigned)d.nbx;
    bx = (int)(b - (long long)row * d.nbx);
    bz = (int)(row / (unsigned)d.nby);
    by = (int)(row - (unsigned long long)bz * d.nby);
}

__device__ inline long long brick_id(const Dims& d, int bx, int by, int bz) { return ((long long)bz * d.nby + by) * d.nbx + bx; }

__device__ inline bool brick_in(const Dims& d, int bx, int by, int bz) {
    return (unsigned)bx < (unsigned)d.nbx && (unsigned)by < (unsigned)d.nby && (unsigned)bz < (unsigned)d.nbz;
}

// ---- the mask from the occupancy grid

__device__ inline uint32_t expand_bits(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}

__device__ inline bool occupied(const uint8_t* __restrict__ bitfield, const Occ& o, int k, int cx, int cy, int cz) {
    const unsigned long long g3 = (unsigned long long)o.G * o.G * o.G;
    const unsigned long long bit = (unsigned long long)k * g3 + (expand_bits(cx) | expand_bits(cy) << 1 | expand_bits(cz) << 2);
    return (bitfield[bit >> 3] >> (bit & 7)) & 1;
}

// cascade and cell box [c0, c1] of a brick, by the header's f64 rule
__device__ inline void brick_cells(const Occ& o, const Dims& d, int bx, int by, int bz, int& k, int c0[3], int c1[3]) {
    const int b[3] = {bx, by, bz}, n[3] = {d.nx, d.ny, d.nz};
    double g0[3], g1[3];
    for (int a = 0; a < 3; ++a) {
        const double e0 = o.lo[a] + (double)(SB * b[a]) * o.h[a];
        const double e1 = o.lo[a] + (double)min(SB * b[a] + SB, n[a] - 1) * o.h[a];
        const double m = o.margin * o.h[a];
        g0[a] = e0 - m;
        g1[a] = e1 + m;
    }
    k = o.cascades - 1;
    for (int c = 0; c < o.cascades; ++c) {
        const double s = fmin(ldexp(1.0, c - 1), o.scale);
        if (-s <= g0[0] && g1[0] <= s && -s <= g0[1] && g1[1] <= s && -s <= g0[2] && g1[2] <= s) {
            k = c;
            break;
        }
    }
    const double s = fmin(ldexp(1.0, k - 1), o.scale);
    const double G = (double)o.G;
    for (int a = 0; a < 3; ++a) {
        c0[a] = (int)fmin(fmax(floor((g0[a] / s + 1.0) * 0.5 * G), 0.0), G - 1.0);
        c1[a] = (int)fmin(fmax(floor((g1[a] / s + 1.0) * 0.5 * G), 0.0), G - 1.0);
    }
}

__global__ __launch_bounds__(IX_THREADS) void sp_mask_small(const uint8_t* __restrict__ bitfield, Occ o, Dims d, uint8_t* __restrict__ mesh_mask) {
    const long long b = (long long)blockIdx.x * IX_THREADS + threadIdx.x;
    if (b >= d.nb) return;
    int bx, by, bz, k, c0[3], c1[3];
    brick_xyz(b, d, bx, by, bz);
    brick_cells(o, d, bx, by, bz, k, c0, c1);
    bool any = false;
    for (int cz = c0[2]; cz <= c1[2]; ++cz)
        for (int cy = c0[1]; cy <= c1[1]; ++cy)
            for (int cx = c0[0]; cx <= c1[0]; ++cx) any |= occupied(bitfield, o, k, cx, cy, cz);
    mesh_mask[b] = any;
}

__global__ __launch_bounds__(IX_THREADS) void sp_mask_box(const uint8_t* __restrict__ bitfield, Occ o, Dims d, uint8_t* __restrict__ mesh_mask) {
    const long long b = blockIdx.x;
    int bx, by, bz, k, c0[3], c1[3];
    brick_xyz(b, d, bx, by, bz);
    brick_cells(o, d, bx, by, bz, k, c0, c1);                  // the same box in every thread
    const int wx = c1[0] - c0[0] + 1, wy = c1[1] - c0[1] + 1, wz = c1[2] - c0[2] + 1;
    const long long cells = (long long)wx * wy * wz;
    int any = 0;
    for (long long e = threadIdx.x; e < cells && !any; e += IX_THREADS) {
        const int cx = c0[0] + (int)(e % wx), cy = c0[1] + (int)((e / wx) % wy), cz = c0[2] + (int)(e / ((long long)wx * wy));
        any = occupied(bitfield, o, k, cx, cy, cz);
    }
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) mesh_mask[b] = any != 0;
}

// ---- dilation, slots and lists

__global__ __launch_bounds__(IX_THREADS) void sp_dilate(const uint8_t* __restrict__ mesh_mask, Dims d, uint8_t* __restrict__ sample_mask,
                                                        int* __restrict__ block_counts) {
    __shared__ int lds4[IX_THREADS / 64];
    const long long base = (long long)blockIdx.x * IX_BLOCK;
    int acc = 0;
    for (int r = 0; r < IX_ITERS; ++r) {
        const long long b = base + r * IX_THREADS + threadIdx.x;
        if (b >= d.nb) break;
        int bx, by, bz;
        brick_xyz(b, d, bx, by, bz);
        int s = 0;
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    if (brick_in(d, bx + dx, by + dy, bz + dz)) s |= mesh_mask[brick_id(d, bx + dx, by + dy, bz + dz)] != 0;
        sample_mask[b] = (uint8_t)s;
        acc += (mesh_mask[b] != 0) | s << 16;
    }
    const int total = block_sum<IX_THREADS>(acc, lds4);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

// exclusive scans of the low and the high half-words of counts[0 .. n): offsets lo_off / hi_off, totals {low, high}
__global__ __launch_bounds__(SCAN_THREADS) void sp_scan_packed(const int* __restrict__ counts, long long n, long long* __restrict__ lo_off,
                                                               long long* __restrict__ hi_off, long long* __restrict__ totals) {
    __shared__ long long s[2][SCAN_THREADS];
    const long long tl = scan_array([=](long long b) { return (long long)(counts[b] & 0xffff); }, n, lo_off, s);
    const long long th = scan_array([=](long long b) { return (long long)(counts[b] >> 16); }, n, hi_off, s);
    if (threadIdx.x == 0) {
        totals[0] = tl;
        totals[1] = th;
    }
}

__global__ __launch_bounds__(IX_THREADS) void sp_index_fill(const uint8_t* __restrict__ mesh_mask, const uint8_t* __restrict__ sample_mask, Dims d,
                                                            const long long* __restrict__ mesh_off, const long long* __restrict__ sample_off,
                                                            long long n_mesh, long long n_sample, int* __restrict__ brick_table,
                                                            int* __restrict__ mesh_bricks, int* __restrict__ sample_bricks) {
    __shared__ int lds4[IX_THREADS / 64];
    const long long base = (long long)blockIdx.x * IX_BLOCK;
    long long cm = mesh_off[blockIdx.x], cs = sample_off[blockIdx.x];
    for (int r = 0; r < IX_ITERS; ++r) {
        const long long b = base + r * IX_THREADS + threadIdx.x;
        const bool live = b < d.nb;                         // block-uniform loop: every thread takes part in the scan
        const int m = live && mesh_mask[b] != 0, s = live && sample_mask[b] != 0;
        int total;
        const int pre = block_exscan<IX_THREADS>(m | s << 16, total, lds4);
        const long long im = cm + (pre & 0xffff), is = cs + (pre >> 16);
        cm += total & 0xffff;
        cs += total >> 16;
        if (!live) continue;
        brick_table[b] = s && is < n_sample ? (int)is : -1;
        if (s && is < n_sample) sample_bricks[is] = (int)b;
        if (m && im < n_mesh) mesh_bricks[im] = (int)b;
    }
}

__global__ __launch_bounds__(IX_THREADS) void sp_points(Dims d, Geom g, const int* __restrict__ sample_bricks, long long begin, long long points,
                                                        float* __restrict__ xyz) {
    const long long s = (long long)blockIdx.x * IX_THREADS + threadIdx.x;
    if (s >= points) return;
    const long long b = sample_bricks[begin + (s >> 9)];
    if ((unsigned long long)b >= (unsigned long long)d.nb) return;
    const int l = (int)(s & (SB3 - 1));
    int bx, by, bz;
    brick_xyz(b, d, bx, by, bz);
    const int idx[3] = {min(SB * bx + (l & 7), d.nx - 1), min(SB * by + (l >> 3 & 7), d.ny - 1), min(SB * bz + (l >> 6), d.nz - 1)};
    for (int a = 0; a < 3; ++a) xyz[3 * s + a] = mc_position(g.lo[a], g.h[a], idx[a]);
}

// ---- marching cubes over the bricks

// Sigma of the points 8 b + LO .. 8 b + LO + DIM - 1 per axis into tile (DIM^3, x fastest), through the sample slots of the 27
// bricks round (bx, by, bz), which it leaves in nslot ((dz + 1)*9 + (dy + 1)*3 + dx + 1; -1: absent).  Points outside the lattice
// and points of bricks that are not sampled read 0: the contract keeps every point that matters sampled.  Closes with a barrier.
template <int LO, int DIM>
__device__ inline void load_tile(const float* __restrict__ pool, const int* __restrict__ brick_table, long long n_sample, const Dims& d, int bx,
                                 int by, int bz, float* __restrict__ tile, int* __restrict__ nslot) {
    static_assert(LO >= -SB && LO + DIM <= 2 * SB, "the tile reaches past the 27 bricks");
    if (threadIdx.x < 27) {
        const int t = threadIdx.x;
        const int gx = bx + t % 3 - 1, gy = by + (t / 3) % 3 - 1, gz = bz + t / 9 - 1;
        int slot = -1;
        if (brick_in(d, gx, gy, gz)) slot = brick_table[brick_id(d, gx, gy, gz)];
        nslot[t] = (unsigned long long)slot < (unsigned long long)n_sample ? slot : -1;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < DIM * DIM * DIM; e += SP_THREADS) {
        const int x = SB * bx + LO + e % DIM, y = SB * by + LO + (e / DIM) % DIM, z = SB * bz + LO + e / (DIM * DIM);
        float v = 0.0f;
        if ((unsigned)x < (unsigned)d.nx && (unsigned)y < (unsigned)d.ny && (unsigned)z < (unsigned)d.nz) {
            const int slot = nslot[((z >> 3) - bz + 1) * 9 + ((y >> 3) - by + 1) * 3 + (x >> 3) - bx + 1];
            if (slot >= 0) v = pool[(long long)slot * SB3 + ((z & 7) * SB + (y & 7)) * SB + (x & 7)];
        }
        tile[e] = v;
    }
    __syncthreads();
}

__global__ __launch_bounds__(SP_THREADS) void sp_count(const float* __restrict__ pool, Dims d, float thr, const uint8_t* __restrict__ mesh_mask,
                                                       const int* __restrict__ brick_table, const int* __restrict__ sample_bricks,
                                                       long long n_sample, uint8_t* __restrict__ flags, int* __restrict__ counts) {
    constexpr int DIM = SB + 1;
    __shared__ float tile[DIM * DIM * DIM];
    __shared__ int nslot[27], meshed[8], lds8[SP_THREADS / 64];
    const long long slot = blockIdx.x;
    const long long b = sample_bricks[slot];
    const int tid = threadIdx.x;
    int bx = 0, by = 0, bz = 0;
    const bool known = (unsigned long long)b < (unsigned long long)d.nb;
    if (known) brick_xyz(b, d, bx, by, bz);
    if (tid < 8) {                                          // the bricks at 0 / -1 per axis: those of the cells round my points' edges
        const int gx = bx - (tid & 1), gy = by - (tid >> 1 & 1), gz = bz - (tid >> 2);
        meshed[tid] = known && brick_in(d, gx, gy, gz) && mesh_mask[brick_id(d, gx, gy, gz)] != 0;
    }
    __syncthreads();
    int any = 0;
    for (int q = 0; q < 8; ++q) any |= meshed[q];
    if (!any) {                                             // (uniform) no vertex and no face here: its flags are never read
        if (tid == 0) counts[slot] = 0;
        return;
    }
    load_tile<0, DIM>(pool, brick_table, n_sample, d, bx, by, bz, tile, nslot);
    const int li = tid & 7, lj = tid >> 3 & 7, lk = tid >> 6;
    const int x = SB * bx + li, y = SB * by + lj, z = SB * bz + lk;
    int in0 = 0, mask = 0, tris = 0;
    if (x < d.nx && y < d.ny && z < d.nz) {
        const auto inside = [&](int dx, int dy, int dz) { return mc_inside(tile[((lk + dz) * DIM + lj + dy) * DIM + li + dx], thr); };
        // is the cell at my point displaced by -(dx, dy, dz) in a meshed brick?  A displaced cell exists when the point is not 0
        const auto cell_meshed = [&](int dx, int dy, int dz) { return meshed[(dx && li == 0) | (dy && lj == 0) << 1 | (dz && lk == 0) << 2]; };
        const bool hx = x + 1 < d.nx, hy = y + 1 < d.ny, hz = z + 1 < d.nz;     // the cells at my coordinate exist along the axis
        const bool px = x > 0, py = y > 0, pz = z > 0;                           // the cells one below exist
        in0 = inside(0, 0, 0);
        const bool ux = hx && ((hy && hz && cell_meshed(0, 0, 0)) || (py && hz && cell_meshed(0, 1, 0)) || (hy && pz && cell_meshed(0, 0, 1)) ||
                               (py && pz && cell_meshed(0, 1, 1)));
        const bool uy = hy && ((hx && hz && cell_meshed(0, 0, 0)) || (px && hz && cell_meshed(1, 0, 0)) || (hx && pz && cell_meshed(0, 0, 1)) ||
                               (px && pz && cell_meshed(1, 0, 1)));
        const bool uz = hz && ((hx && hy && cell_meshed(0, 0, 0)) || (px && hy && cell_meshed(1, 0, 0)) || (hx && py && cell_meshed(0, 1, 0)) ||
                               (px && py && cell_meshed(1, 1, 0)));
        if (ux) mask |= inside(1, 0, 0) != in0;
        if (uy) mask |= (inside(0, 1, 0) != in0) << 1;
        if (uz) mask |= (inside(0, 0, 1) != in0) << 2;
        if (hx && hy && hz && meshed[0]) tris = NGP_MC_TRI_COUNT[mc_cube([&](int c) { return inside(c & 1, c >> 1 & 1, c >> 2); })];
    }
    flags[slot * SB3 + tid] = (uint8_t)(in0 | mask << 1);
    const int total = block_sum<SP_THREADS>((int)__popc(mask) | tris << 16, lds8);   // of the packed counts (fits: static_assert above)
    if (tid == 0) counts[slot] = total;
}

__global__ __launch_bounds__(SP_THREADS) void sp_emit_vertices(const float* __restrict__ pool, Dims d, float thr, Geom g,
                                                               const int* __restrict__ brick_table, const int* __restrict__ sample_bricks,
                                                               long long n_sample, const uint8_t* __restrict__ flags,
                                                               const int* __restrict__ counts, const long long* __restrict__ vertex_off,
                                                               int* __restrict__ voff, long long cap, float* __restrict__ verts,
                                                               float* __restrict__ normals, long long* __restrict__ keys) {
    constexpr int DIM = SB + 3;
    __shared__ float tile[DIM * DIM * DIM];
    __shared__ int nslot[27], lds8[SP_THREADS / 64];
    const long long slot = blockIdx.x;
    if ((counts[slot] & 0xffff) == 0) return;               // (uniform) owns no vertex: sp_count wrote no flags either
    const long long b = sample_bricks[slot];
    const int tid = threadIdx.x;
    int bx, by, bz;
    brick_xyz(b, d, bx, by, bz);                            // in range: sp_count counted nothing for a brick that is not
    load_tile<-1, DIM>(pool, brick_table, n_sample, d, bx, by, bz, tile, nslot);
    const int mask = flags[slot * SB3 + tid] >> 1;
    int total;
    long long vi = vertex_off[slot] + block_exscan<SP_THREADS>((int)__popc(mask), total, lds8);
    voff[slot * SB3 + tid] = (int)vi;                       // fits: the caller's total is <= INT32_MAX (ngp_meshsparse_emit)
    if (!mask) return;
    const int l[3] = {tid & 7, tid >> 3 & 7, tid >> 6};
    const int idx[3] = {SB * bx + l[0], SB * by + l[1], SB * bz + l[2]};
    const int n[3] = {d.nx, d.ny, d.nz};
    const auto sigma = [&](int dx, int dy, int dz) { return tile[((l[2] + 1 + dz) * DIM + l[1] + 1 + dy) * DIM + l[0] + 1 + dx]; };
    // gradient at my point displaced by o
    const auto gradient = [&](int ox, int oy, int oz, float out[3]) {
        out[0] = mc_grad_axis([&](int s) { return sigma(ox + s, oy, oz); }, idx[0] + ox, n[0], g.h[0]);
        out[1] = mc_grad_axis([&](int s) { return sigma(ox, oy + s, oz); }, idx[1] + oy, n[1], g.h[1]);
        out[2] = mc_grad_axis([&](int s) { return sigma(ox, oy, oz + s); }, idx[2] + oz, n[2], g.h[2]);
    };
    const float sa = sigma(0, 0, 0);
    float pa[3], ga[3];
    for (int a = 0; a < 3; ++a) pa[a] = mc_position(g.lo[a], g.h[a], idx[a]);
    gradient(0, 0, 0, ga);
    const long long p = ((long long)idx[2] * d.ny + idx[1]) * d.nx + idx[0];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(mask >> a & 1)) continue;
        const int ox = a == 0, oy = a == 1, oz = a == 2;
        const float t = mc_edge_t(thr, sa, sigma(ox, oy, oz));
        float gb[3];
        gradient(ox, oy, oz, gb);
        if (vi < cap) {
            mc_vertex(pa, a, mc_position(g.lo[a], g.h[a], idx[a] + 1), t, ga, gb, verts + 3 * vi, normals ? normals + 3 * vi : nullptr);
            if (keys) keys[vi] = 3 * p + a;
        }
        ++vi;
    }
}

__global__ __launch_bounds__(SP_THREADS) void sp_emit_faces(const float* __restrict__ pool, Dims d, float thr, const int* __restrict__ brick_table,
                                                            const int* __restrict__ mesh_bricks, long long n_sample,
                                                            const uint8_t* __restrict__ flags, const int* __restrict__ voff,
                                                            const long long* __restrict__ face_off, long long cap, int* __restrict__ faces,
                                                            long long* __restrict__ cells) {
    constexpr int DIM = SB + 1;
    __shared__ float tile[DIM * DIM * DIM];
    __shared__ int nslot[27], lds8[SP_THREADS / 64];
    const long long b = mesh_bricks[blockIdx.x];
    if ((unsigned long long)b >= (unsigned long long)d.nb) return;      // (uniform)
    const int tid = threadIdx.x;
    int bx, by, bz;
    brick_xyz(b, d, bx, by, bz);
    load_tile<0, DIM>(pool, brick_table, n_sample, d, bx, by, bz, tile, nslot);
    const int mine = nslot[13];
    if (mine < 0) return;                                   // (uniform) a meshed brick is sampled
    const int li = tid & 7, lj = tid >> 3 & 7, lk = tid >> 6;
    const int x = SB * bx + li, y = SB * by + lj, z = SB * bz + lk;
    int cube = 0;
    if (x + 1 < d.nx && y + 1 < d.ny && z + 1 < d.nz)
        cube = mc_cube([&](int c) { return mc_inside(tile[((lk + (c >> 2)) * DIM + lj + (c >> 1 & 1)) * DIM + li + (c & 1)], thr); });
    const int nt = NGP_MC_TRI_COUNT[cube];
    int total;
    const long long f0 = face_off[mine] + block_exscan<SP_THREADS>(nt, total, lds8);
    const long long p = ((long long)z * d.ny + y) * d.nx + x;
    for (int tr = 0; tr < nt; ++tr) {
        if (f0 + tr >= cap) break;
        for (int k = 0; k < 3; ++k) {
            int corner, axis;
            mc_face_corner(cube, tr, k, corner, axis);
            const int ox = li + (corner & 1), oy = lj + (corner >> 1 & 1), oz = lk + (corner >> 2);      // 0 .. 8: mine or a brick at +1
            const int slot = nslot[((oz >> 3) + 1) * 9 + ((oy >> 3) + 1) * 3 + (ox >> 3) + 1];
            int v = -1;
            if (slot >= 0) {
                const long long q = (long long)slot * SB3 + ((oz & 7) * SB + (oy & 7)) * SB + (ox & 7);
                v = voff[q] + __popc((flags[q] >> 1) & ((1 << axis) - 1));
            }
            faces[3 * (f0 + tr) + k] = v;
        }
        if (cells) cells[f0 + tr] = p;
    }
}

// ---- host

bool dims_ok(int nx, int ny, int nz, Dims& d) {
    if (nx < 2 || ny < 2 || nz < 2 || nx > MAX_AXIS || ny > MAX_AXIS || nz > MAX_AXIS) return false;
    d.nx = nx;
    d.ny = ny;
    d.nz = nz;
    d.nbx = (nx + SB - 1) / SB;
    d.nby = (ny + SB - 1) / SB;
    d.nbz = (nz + SB - 1) / SB;
    d.nb = (long long)d.nbx * d.nby * d.nbz;
    return d.nb <= MAX_BRICKS;
}

bool bounds_ok(const float* b6) {
    for (int a = 0; a < 3; ++a)
        if (!(b6[3 + a] > b6[a]) || !(b6[3 + a] - b6[a] < 3.0e38f)) return false;      // also rejects NaN and infinities
    return true;
}

void geom_of(const Dims& d, const float* b6, Geom& g) {
    const int n[3] = {d.nx, d.ny, d.nz};
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = b6[a];
        g.h[a] = (b6[3 + a] - b6[a]) / (float)(n[a] - 1);
    }
}

struct IndexLayout {
    size_t sample, counts, mesh_off, sample_off, total;
    long long blocks;
};

IndexLayout index_layout(const Dims& d) {
    IndexLayout l;
    l.blocks = blocks_of(d.nb, IX_BLOCK);
    l.sample = 0;
    l.counts = align256((size_t)d.nb);
    l.mesh_off = l.counts + align256((size_t)l.blocks * 4);
    l.sample_off = l.mesh_off + align256((size_t)l.blocks * 8);
    l.total = l.sample_off + align256((size_t)l.blocks * 8);
    return l;
}

struct Layout {
    size_t flags, voff, counts, vertex_off, face_off, total;
};

bool slots_ok(int64_t n_mesh, int64_t n_sample) { return n_sample >= 1 && n_sample <= MAX_BRICKS && n_mesh >= 0 && n_mesh <= n_sample; }

Layout layout(long long n_sample) {
    Layout l;
    l.flags = 0;
    l.voff = align256((size_t)n_sample * SB3);
    l.counts = l.voff + align256((size_t)n_sample * SB3 * 4);
    l.vertex_off = l.counts + align256((size_t)n_sample * 4);
    l.face_off = l.vertex_off + align256((size_t)n_sample * 8);
    l.total = l.face_off + align256((size_t)n_sample * 8);
    return l;
}

}  // namespace

NGP_API int ngp_meshsparse_abi_version(void) { return 1; }

NGP_API const char* ngp_meshsparse_build_arch(void) { return "gfx950"; }

NGP_API int ngp_meshsparse_mask(const uint8_t* density_bitfield, int cascades, int grid_size, float scale, int nx, int ny, int nz,
                                const float* bounds6, double margin_voxels, uint8_t* mesh_mask, void* stream) {
    Dims d;
    if (!dims_ok(nx, ny, nz, d) || !density_bitfield || !bounds6 || !mesh_mask || !bounds_ok(bounds6)) return NGP_EINVAL;
    if (cascades < 1 || cascades > 32 || grid_size < 2 || grid_size > 1024 || (grid_size & (grid_size - 1))) return NGP_EINVAL;
    if (!(scale > 0.f) || !(scale <= 3.0e38f) || !(margin_voxels >= 0.0) || !(margin_voxels <= 1.0e6)) return NGP_EINVAL;
    Occ o;
    const int n[3] = {nx, ny, nz};
    bool small = true;
    const double cell0 = 2.0 * fmin(0.5, (double)scale) / grid_size;        // the smallest occupancy cell
    for (int a = 0; a < 3; ++a) {
        o.lo[a] = (double)bounds6[a];
        o.h[a] = ((double)bounds6[3 + a] - (double)bounds6[a]) / (double)(n[a] - 1);
        small = small && (SB + 2.0 * margin_voxels) * o.h[a] <= cell0;      // a grown brick then meets at most two cells along the axis
    }
    o.margin = margin_voxels;
    o.scale = (double)scale;
    o.cascades = cascades;
    o.G = grid_size;
    hipStream_t s = (hipStream_t)stream;
    if (small)
        hipLaunchKernelGGL(sp_mask_small, dim3((unsigned)blocks_of(d.nb, IX_THREADS)), dim3(IX_THREADS), 0, s, density_bitfield, o, d, mesh_mask);
    else
        hipLaunchKernelGGL(sp_mask_box, dim3((unsigned)d.nb), dim3(IX_THREADS), 0, s, density_bitfield, o, d, mesh_mask);
    return launched();
}

NGP_API size_t ngp_meshsparse_index_workspace_bytes(int nx, int ny, int nz) {
    Dims d;
    if (!dims_ok(nx, ny, nz, d)) return 0;
    return index_layout(d).total;
}

NGP_API int ngp_meshsparse_index_count(const uint8_t* mesh_mask, int nx, int ny, int nz, void* workspace, size_t workspace_bytes,
                                       int64_t* counts, void* stream) {
    Dims d;
    if (!dims_ok(nx, ny, nz, d) || !mesh_mask || !workspace || !counts) return NGP_EINVAL;
    const IndexLayout l = index_layout(d);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sp_dilate, dim3((unsigned)l.blocks), dim3(IX_THREADS), 0, s, mesh_mask, d, (uint8_t*)(ws + l.sample), (int*)(ws + l.counts));
    hipLaunchKernelGGL(sp_scan_packed, dim3(1), dim3(SCAN_THREADS), 0, s, (const int*)(ws + l.counts), l.blocks, (long long*)(ws + l.mesh_off),
                       (long long*)(ws + l.sample_off), (long long*)counts);
    return launched();
}

NGP_API int ngp_meshsparse_index_fill(const uint8_t* mesh_mask, int nx, int ny, int nz, void* workspace, size_t workspace_bytes,
                                      int64_t n_mesh, int64_t n_sample, int32_t* brick_table, int32_t* mesh_bricks, int32_t* sample_bricks,
                                      void* stream) {
    Dims d;
    if (!dims_ok(nx, ny, nz, d) || !mesh_mask || !workspace || !brick_table) return NGP_EINVAL;
    if (n_mesh < 0 || n_sample < n_mesh || n_sample > d.nb || (n_mesh > 0 && !mesh_bricks) || (n_sample > 0 && !sample_bricks)) return NGP_EINVAL;
    const IndexLayout l = index_layout(d);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    char* ws = (char*)workspace;
    hipLaunchKernelGGL(sp_index_fill, dim3((unsigned)l.blocks), dim3(IX_THREADS), 0, (hipStream_t)stream, mesh_mask, (const uint8_t*)(ws + l.sample),
                       d, (const long long*)(ws + l.mesh_off), (const long long*)(ws + l.sample_off), (long long)n_mesh, (long long)n_sample,
                       brick_table, mesh_bricks, sample_bricks);
    return launched();
}

NGP_API int ngp_meshsparse_points(int nx, int ny, int nz, const float* bounds6, const int32_t* sample_bricks, int64_t n_sample, int64_t begin,
                                  int64_t count, float* xyz, void* stream) {
    Dims d;
    if (!dims_ok(nx, ny, nz, d) || !bounds6 || n_sample < 0 || n_sample > d.nb || begin < 0 || count < 0 || begin > n_sample ||
        count > n_sample - begin)
        return NGP_EINVAL;
    if (count == 0) return 0;
    if (!sample_bricks || !xyz || !bounds_ok(bounds6)) return NGP_EINVAL;
    Geom g;
    geom_of(d, bounds6, g);
    const long long points = (long long)count * SB3;
    hipLaunchKernelGGL(sp_points, dim3((unsigned)blocks_of(points, IX_THREADS)), dim3(IX_THREADS), 0, (hipStream_t)stream, d, g, sample_bricks,
                       (long long)begin, points, xyz);
    return launched();
}

NGP_API size_t ngp_meshsparse_workspace_bytes(int64_t n_mesh, int64_t n_sample) {
    if (!slots_ok(n_mesh, n_sample)) return 0;
    return layout(n_sample).total;
}

NGP_API int ngp_meshsparse_count(const float* pool, int nx, int ny, int nz, float threshold, const uint8_t* mesh_mask,
                                 const int32_t* brick_table, const int32_t* mesh_bricks, int64_t n_mesh, const int32_t* sample_bricks,
                                 int64_t n_sample, void* workspace, size_t workspace_bytes, int64_t* totals, void* stream) {
    Dims d;
    if (!dims_ok(nx, ny, nz, d) || !slots_ok(n_mesh, n_sample) || n_sample > d.nb) return NGP_EINVAL;
    if (!pool || !mesh_mask || !brick_table || !sample_bricks || (n_mesh > 0 && !mesh_bricks) || !workspace || !totals) return NGP_EINVAL;
    const Layout l = layout(n_sample);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sp_count, dim3((unsigned)n_sample), dim3(SP_THREADS), 0, s, pool, d, threshold, mesh_mask, brick_table, sample_bricks,
                       (long long)n_sample, (uint8_t*)(ws + l.flags), (int*)(ws + l.counts));
    hipLaunchKernelGGL(sp_scan_packed, dim3(1), dim3(SCAN_THREADS), 0, s, (const int*)(ws + l.counts), (long long)n_sample,
                       (long long*)(ws + l.vertex_off), (long long*)(ws + l.face_off), (long long*)totals);
    return launched();
}

NGP_API int ngp_meshsparse_emit(const float* pool, int nx, int ny, int nz, float threshold, const float* bounds6, const int32_t* brick_table,
                                const int32_t* mesh_bricks, int64_t n_mesh, const int32_t* sample_bricks, int64_t n_sample, void* workspace,
                                size_t workspace_bytes, int64_t n_vertices, int64_t n_faces, float* vertices, float* normals, int64_t* vertex_key,
                                int32_t* faces, int64_t* face_cell, void* stream) {
    Dims d;
    if (!dims_ok(nx, ny, nz, d) || !slots_ok(n_mesh, n_sample) || n_sample > d.nb || n_vertices < 0 || n_faces < 0) return NGP_EINVAL;
    if (!pool || !bounds6 || !brick_table || !sample_bricks || (n_mesh > 0 && !mesh_bricks) || !workspace) return NGP_EINVAL;
    if ((n_vertices > 0 && !vertices) || (n_faces > 0 && !faces) || !bounds_ok(bounds6)) return NGP_EINVAL;
    if (n_vertices > INT32_MAX || n_faces > INT32_MAX) return NGP_ERANGE;
    const Layout l = layout(n_sample);
    if (workspace_bytes < l.total) return NGP_EINVAL;
    if (n_vertices == 0 && n_faces == 0) return 0;
    Geom g;
    geom_of(d, bounds6, g);
    char* ws = (char*)workspace;
    hipStream_t s = (hipStream_t)stream;
    // the vertices first, also when the caller wants none: the faces read the vertex offsets they leave
    hipLaunchKernelGGL(sp_emit_vertices, dim3((unsigned)n_sample), dim3(SP_THREADS), 0, s, pool, d, threshold, g, brick_table, sample_bricks,
                       (long long)n_sample, (const uint8_t*)(ws + l.flags), (const int*)(ws + l.counts), (const long long*)(ws + l.vertex_off),
                       (int*)(ws + l.voff), (long long)n_vertices, vertices, normals, (long long*)vertex_key);
    if (n_faces > 0 && n_mesh > 0)
        hipLaunchKernelGGL(sp_emit_faces, dim3((unsigned)n_mesh), dim3(SP_THREADS), 0, s, pool, d, threshold, brick_table, mesh_bricks,
                           (long long)n_sample, (const uint8_t*)(ws + l.flags), (const int*)(ws + l.voff), (const long long*)(ws + l.face_off),
                           (long long)n_faces, faces, (long long*)face_cell);
    return launched();
}
