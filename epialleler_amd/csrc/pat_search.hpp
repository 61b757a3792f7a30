// The searches behind a flat list of (target, candidate row) pairs, shared by the pattern calls (patterns.hip) and the
// region report (region_report.hip): the ranges of candidate rows of the targets, laid end to end under the u64 exclusive
// scan pre[], and the first row at or behind a (rname, start) key in rows sorted by it.  Device code only.
#pragma once
#include "common.hpp"

namespace epi {

// last t in [a, b) with key(t) <= v, for keys that do not decrease and key(a) <= v; at most 32 steps
template <class V, class Key> __device__ __forceinline__ int32_t pat_last_le(int32_t a, int32_t b, V v, Key key) {
  for (int it = 0; it < 32 && b - a > 1; it++) {
    const int32_t m = a + ((b - a) >> 1);
    if (key(m) <= v) a = m; else b = m;
  }
  return a;
}

// the target of pair j (pre[0] = 0 <= j < pre[ng])
__device__ __forceinline__ int32_t pat_target_of(const uint64_t *__restrict__ pre, int32_t ng, uint64_t j) {
  return pat_last_le(0, ng, j, [&](int32_t t) { return pre[t]; });
}

// first row in [0, n) with (rname, start) >= (qr, qp); at most 64 steps
__device__ __forceinline__ int64_t pat_row_lower_bound(const int32_t *__restrict__ rname, const int32_t *__restrict__ start, int64_t n,
                                                       int32_t qr, int64_t qp) {
  int64_t a = 0, b = n;
  for (int it = 0; it < 64 && a < b; it++) {
    const int64_t m = a + ((b - a) >> 1);
    const int32_t r = rname[m];
    if (r < qr || (r == qr && (int64_t)start[m] < qp)) a = m + 1; else b = m;
  }
  return a;
}

}  // namespace epi
