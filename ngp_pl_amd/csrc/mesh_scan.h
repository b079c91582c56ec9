// Integer sums and prefix sums of the mesh stages, once: over a wave, over a workgroup, and over an array by one workgroup.  Included
// inside the including library's anonymous namespace, as mesh_compact.h is.  T is int or long long; integer sums do not depend on
// their order, so every result is exact.
//   wave_sum, wave_incscan        across the 64 lanes, in registers;
//   block_sum, block_exscan       across the WG threads of the workgroup: the wave forms, then the WG / 64 wave totals through LDS
//                                 words the caller supplies.  Block-uniform, and both close with a barrier: the words are free again;
//   scan_array                    exclusive int64 scan of any number of items by one workgroup of SCAN_THREADS.
#ifndef NGP_MESH_SCAN_H
#define NGP_MESH_SCAN_H

constexpr int SCAN_THREADS = 1024;

template <class T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// inclusive prefix of x over the lanes of the wave
template <class T>
__device__ __forceinline__ T wave_incscan(T x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

// sum of acc over the WG threads of the block, to every thread
template <int WG, class T>
__device__ __forceinline__ T block_sum(T acc, T* lds) {
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
    __syncthreads();
    T total = 0;
#pragma unroll
    for (int q = 0; q < WG / 64; ++q) total += lds[q];
    __syncthreads();
    return total;
}

// exclusive prefix of v over the WG threads of the block, and the block total
template <int WG, class T>
__device__ __forceinline__ T block_exscan(T v, T& total, T* lds) {
    const int w = threadIdx.x >> 6;
    const T x = wave_incscan(v);
    if ((threadIdx.x & 63) == 63) lds[w] = x;
    __syncthreads();
    T pre = 0;
    total = 0;
#pragma unroll
    for (int q = 0; q < WG / 64; ++q) {
        const T s = lds[q];
        pre += q < w ? s : 0;
        total += s;
    }
    __syncthreads();
    return pre + x - v;
}

// Exclusive int64 scan of item(0), ..., item(n - 1) into offsets[0], ..., offsets[n - 1] by the whole workgroup of SCAN_THREADS;
// returns the total to every thread.  A serial run per thread, Hillis-Steele over the per-thread sums, a serial write-out.  A thread
// reads an item before it writes that item's offset and touches no other thread's items: item may read the words offsets writes.
// Closes with a barrier: s is free again and the workgroup sees the offsets.
template <class Item>
__device__ __forceinline__ long long scan_array(Item item, long long n, long long* offsets, long long (*s)[SCAN_THREADS]) {
    const int t = threadIdx.x;
    const long long per = (n + SCAN_THREADS - 1) / SCAN_THREADS;
    const long long b0 = min(n, t * per), b1 = min(n, b0 + per);
    long long mine = 0;
    for (long long b = b0; b < b1; ++b) mine += item(b);
    int cur = 0;
    s[0][t] = mine;
    __syncthreads();
    for (int o = 1; o < SCAN_THREADS; o <<= 1) {        // inclusive Hillis-Steele over the per-thread sums
        long long a = s[cur][t];
        if (t >= o) a += s[cur][t - o];
        s[cur ^ 1][t] = a;
        cur ^= 1;
        __syncthreads();
    }
    long long off = s[cur][t] - mine;
    for (long long b = b0; b < b1; ++b) {
        const long long c = item(b);
        offsets[b] = off;
        off += c;
    }
    const long long total = s[cur][SCAN_THREADS - 1];
    __syncthreads();
    return total;
}

#endif
