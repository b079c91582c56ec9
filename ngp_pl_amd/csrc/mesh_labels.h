// The lanes of a wave grouped by an integer label, once.  Included inside the including library's anonymous namespace, as
// mesh_compact.h is.  Every lane of the wave calls these (a lane without a label passes l < 0): the loop's trip count comes from
// ballots, so it is wave-uniform, and the ballots and shuffles inside it read every lane.
#ifndef NGP_MESH_LABELS_H
#define NGP_MESH_LABELS_H

#include "mesh_scan.h"

constexpr int FOLD_MIN = 8;                             // lanes of one label from which the wave sums before it adds

// f(label, the lanes that hold it, the first of them), once per distinct label l >= 0 present in the wave
template <class F>
__device__ __forceinline__ void for_each_label(int l, F f) {
    unsigned long long todo = __ballot(l >= 0);
    while (todo) {
        const int first = __ffsll((long long)todo) - 1;
        const int cur = __shfl(l, first, 64);
        const unsigned long long same = __ballot(l == cur);
        f(cur, same, first);
        todo &= ~same;
    }
}

// Inside for_each_label: the lanes `same` of one label (mine: this lane is one of them) add val[0..N) to dst[0..N).  FOLD_MIN lanes
// or more are summed across the wave and added by the first lane (a heavy label would otherwise serialise up to 64 adds per
// instruction on one address); fewer add lane by lane.  Zeros are not added.
template <int N>
__device__ __forceinline__ void add_group(bool mine, unsigned long long same, int first, const long long* val, unsigned long long* dst) {
    if (__popcll(same) >= FOLD_MIN) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const long long t = wave_sum(mine ? val[i] : 0);
            if ((int)(threadIdx.x & 63) == first && t) atomicAdd(dst + i, (unsigned long long)t);
        }
    } else if (mine) {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (val[i]) atomicAdd(dst + i, (unsigned long long)val[i]);
    }
}

// adds val[0..N) of every lane with l >= 0 to dst_base[stride * l + first_sum + i]
template <int N>
__device__ __forceinline__ void add_by_label(int l, const long long* val, unsigned long long* dst_base, int stride, int first_sum) {
    for_each_label(l, [&](int cur, unsigned long long same, int first) {
        add_group<N>(l == cur, same, first, val, dst_base + (size_t)stride * (unsigned)cur + first_sum);
    });
}

#endif
