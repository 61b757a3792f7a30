// The series order of a CX table and its cuts, as the smoother (smooth.hip) and the segmentation (segment.hip) both use them:
// the rows are ordered by class (strand - 1) * 8 + context, stably, so a class ascends in (rname, pos); a cluster (the
// smoother's word) or chain (the segmentation's) starts at a class change, at an rname change, or where pos - previous pos >
// max_gap.  The step into series order is shared whole (series_sort); each caller has its own kernel around the head rule (they gather different things).
#pragma once
#include "cx_table.hpp"
#include "radix_sort.hpp"

namespace epi {

constexpr int SERIES_WG = 256;

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

static __global__ __launch_bounds__(SERIES_WG) void k_series_key(CxTab t, uint64_t *__restrict__ key, uint32_t *__restrict__ val,
                                                                 uint32_t *__restrict__ unsorted, uint32_t *__restrict__ bad) {
  const uint32_t i = blockIdx.x * (uint32_t)SERIES_WG + threadIdx.x;
  if (i >= t.n) return;
  key[i] = series_key(t, i, unsorted, bad);
  val[i] = i;
}

// The rows of t into series order, in a SortPairs the caller has placed: (class byte, row) pairs from k_series_key (static: a copy
// per unit), one stable pass over the class byte, inside the profiling range `prof`.  Queued on s; *unsorted and *bad (zeroed by the
// caller) travel in its next read of its scalars.  Then sort.vals() is the rows in series order, sort.keys() their classes.
inline int series_sort(const CxTab &t, SortPairs &sort, uint32_t *unsorted, uint32_t *bad, DevBuf &scan_tmp, const char *prof, hipStream_t s) {
  prof_begin(prof, s);
  hipLaunchKernelGGL(k_series_key, dim3((t.n + SERIES_WG - 1) / SERIES_WG), dim3(SERIES_WG), 0, s, t, sort.keys_in(), sort.vals_in(), unsorted, bad);
  const int rc = sort.sort(0x1u, scan_tmp, s);
  prof_end(prof, s);
  EPI_HIP(hipGetLastError());
  return rc;
}

inline int series_verdict(const char *who, uint32_t unsorted, uint32_t bad) {
  if (unsorted) return fail(EPI_ERR_ARG, "%s: the rows of the table are not strictly ascending in (rname, pos, strand)", who);
  return bad ? fail(EPI_ERR_ARG, "%s: a row has a negative pos, a strand other than 1 and 2, a context code outside 0 .. 7 or a negative count", who) : EPI_OK;
}

}  // namespace epi
