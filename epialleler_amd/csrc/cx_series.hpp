// The series order of a CX table and its cuts, as the smoother (smooth.hip) and the segmentation (segment.hip) both use them:
// the rows are ordered by class (strand - 1) * 8 + context, stably, so a class ascends in (rname, pos); a cluster (the
// smoother's word) or chain (the segmentation's) starts at a class change, at an rname change, or where pos - previous pos >
// max_gap.  Device code; each caller has its own kernels around the two rules.
#pragma once
#include "cx_table.hpp"

namespace epi {

// Row i of the table: *unsorted is set when it is not strictly above row i - 1, *bad when its strand is not 1 or 2, its context
// code is outside 0 .. 7, or pos, meth or unmeth is negative.  Returns the row's class, the sort key.
__device__ __forceinline__ uint64_t series_key(const CxTab &t, uint32_t i, uint32_t *unsorted, uint32_t *bad) {
  const int32_t strand = t.strand[i], ctx = t.context[i];
  if (i > 0 && !cx_above(t, i)) atomicOr(unsorted, 1u);
  if ((strand != 1 && strand != 2) || ctx < 0 || ctx > 7 || t.pos[i] < 0 || t.meth[i] < 0 || t.unmeth[i] < 0) atomicOr(bad, 1u);
  return (uint64_t)((((uint32_t)(strand - 1) & 1u) << 3) | ((uint32_t)ctx & 7u));
}

// Site s of the series order (key: the sorted classes, ord: the rows in series order; row = ord[s], pos = t.pos[row]): 1 when
// it is the first of a cluster or chain.
__device__ __forceinline__ uint32_t series_head(const CxTab &t, const uint64_t *__restrict__ key, const uint32_t *__restrict__ ord, uint32_t s,
                                                uint32_t row, int32_t pos, int32_t max_gap) {
  if (s == 0) return 1u;
  const uint32_t prev = ord[s - 1];
  return key[s] != key[s - 1] || t.rname[prev] != t.rname[row] || (int64_t)pos - (int64_t)t.pos[prev] > (int64_t)max_gap ? 1u : 0u;
}

inline const char *series_unsorted_message() { return "%s: the rows of the table are not strictly ascending in (rname, pos, strand)"; }
inline const char *series_bad_message() {
  return "%s: a row has a negative pos, a strand other than 1 and 2, a context code outside 0 .. 7 or a negative count";
}

}  // namespace epi
