// A caller's CX table as the stateless comparisons (cx_compare.hip, cx_groups.hip) see it, and the order both require of it:
// rows strictly ascending in (rname, pos, strand).
#pragma once
#include "common.hpp"

namespace epi {

struct CxTab {                         // a CX table: rname, strand, pos, context, meth, unmeth
  const int32_t *rname, *strand, *pos, *context, *meth, *unmeth;
  uint32_t n;
};

inline CxTab cx_tab(const int32_t *const d[6], int64_t n) {
  CxTab t;
  t.rname = d[0]; t.strand = d[1]; t.pos = d[2]; t.context = d[3]; t.meth = d[4]; t.unmeth = d[5];
  t.n = (uint32_t)n;
  return t;
}

// row i of t against the key (rname, pos, strand): < 0, 0, > 0
__device__ __forceinline__ int cx_cmp(const CxTab &t, uint32_t i, int32_t rname, int32_t pos, int32_t strand) {
  const int32_t r = t.rname[i];
  if (r != rname) return r < rname ? -1 : 1;
  const int32_t p = t.pos[i];
  if (p != pos) return p < pos ? -1 : 1;
  const int32_t s = t.strand[i];
  return s < strand ? -1 : s > strand ? 1 : 0;
}

// row i (i >= 1) is strictly above row i - 1
__device__ __forceinline__ bool cx_above(const CxTab &t, uint32_t i) { return cx_cmp(t, i - 1, t.rname[i], t.pos[i], t.strand[i]) < 0; }

}  // namespace epi
