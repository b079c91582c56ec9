// splitmix64's finaliser, the hash of the 64-bit keys of the mesh stages' open-addressing tables.  Included inside the including
// library's anonymous namespace, as mesh_compact.h is.
#ifndef NGP_MESH_MIX_H
#define NGP_MESH_MIX_H

__device__ inline unsigned long long mix(unsigned long long x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

#endif
