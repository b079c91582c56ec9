// Host helpers of the mesh stages' C entry points, once.  Included inside the including library's anonymous namespace, as
// mesh_compact.h is.
#ifndef NGP_MESH_HOST_H
#define NGP_MESH_HOST_H

#define NGP_API extern "C" __attribute__((visibility("default")))

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline long long blocks_of(long long n, long long per) { return (n + per - 1) / per; }

inline bool sizes_ok(int64_t n_v, int64_t n_f) { return n_v >= 0 && n_f >= 0 && n_v <= INT32_MAX && n_f <= INT32_MAX; }

inline bool cell_ok(float cell) { return cell > 0.f && cell <= 3.402823466e38f; }

// the error of the launches since the last check, as the C ABI's int
inline int launched() { return (int)hipGetLastError(); }

#endif
