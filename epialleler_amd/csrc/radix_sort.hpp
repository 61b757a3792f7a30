// Stable LSD radix sort of (64-bit key, 32-bit value) pairs (radix_sort.hip has the kernels), and the one workspace type its
// callers place in their scratch: the p-value adjustment (p_adjust.hip), the FDRP report's site -> rows index (fdrp.hip), the
// allele-specific report's events (asm_report.hip), the group comparison's rows (cx_groups.hip) and cx_series.hpp's series order.
#pragma once
#include "common.hpp"

namespace epi {

constexpr int RSORT_WG = 256;
constexpr int RSORT_WAVES = RSORT_WG / 64;
constexpr int RSORT_ITEMS = 16;                                // keys per thread of a sorting pass
constexpr int RSORT_WAVE_KEYS = 64 * RSORT_ITEMS;              // consecutive keys a wave owns
constexpr int RSORT_TILE = RSORT_WG * RSORT_ITEMS;             // 4096 keys per workgroup

constexpr int64_t radix_sort_blocks(int64_t n) { return (n + RSORT_TILE - 1) / RSORT_TILE; }

// The buffers of one sort of n pairs, n < 2^32: two key and two value buffers, between which the pairs bounce, and two
// [digit][workgroup] tables (the passes' histogram and its scan).  It owns nothing: the caller provides bytes(n) bytes, 8-byte
// aligned, and the pieces lie in them in the order key, key, value, value, table, table, every one naturally aligned.
struct SortPairs {
  static size_t pair_bytes(size_t n) { return n * 24; }                                        // the (key, value) buffers
  static size_t table_words(size_t n) { return 256 * (size_t)radix_sort_blocks((int64_t)n); }  // of one table: what a pass scans
  static size_t bytes(size_t n) { return pair_bytes(n) + 2 * 4 * table_words(n); }             // ... and the two tables

  SortPairs(void *mem, size_t n_) : n((uint32_t)n_) {
    key[0] = static_cast<uint64_t *>(mem); key[1] = key[0] + n_;
    val[0] = reinterpret_cast<uint32_t *>(key[1] + n_); val[1] = val[0] + n_;
    table[0] = val[1] + n_; table[1] = table[0] + table_words(n_);
  }
  uint64_t *keys_in() const { return key[0]; }                 // the caller writes its pairs here, then sorts
  uint32_t *vals_in() const { return val[0]; }
  // One pass per set bit d of `byte_mask` (key byte d, least significant first); scan_tmp: the scratch of the scan over the
  // table.  Everything is queued on s, nothing is synchronised.
  int sort(uint32_t byte_mask, DevBuf &scan_tmp, hipStream_t s);
  const uint64_t *keys() const { return key[cur]; }            // the result ...
  const uint32_t *vals() const { return val[cur]; }
  template <class T> T *spare() const { return reinterpret_cast<T *>(key[cur ^ 1]); }   // ... and the 8 n bytes nothing reads after it

 private:
  uint64_t *key[2];
  uint32_t *val[2], *table[2];
  uint32_t n;
  int cur = 0;                                                 // the buffer pair that holds the pairs
};

// one LDS add per lane, or one per wave when every active lane holds the same bin (the exponent bytes of a p-value column)
__device__ __forceinline__ void hist_add(uint32_t *hist, uint32_t bin, bool active, uint64_t amask) {
  if (amask == 0) return;                                                     // (uniform)
  const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)bin, __ffsll((unsigned long long)amask) - 1);
  if (__all(!active || bin == first)) {
    if ((threadIdx.x & 63) == 0) atomicAdd(&hist[first], (uint32_t)__popcll(amask));
  } else if (active) {
    atomicAdd(&hist[bin], 1u);
  }
}

}  // namespace epi
