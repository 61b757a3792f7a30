// Searches over a site list sorted by (rname code, pos), shared by the kernels that enumerate (row, site) pairs from the rows'
// side: the base frequencies (base_freqs.hip) and the allele-specific methylation report (asm_report.hip).
#pragma once
#include "common.hpp"

namespace epi {

// (rname, pos) as one monotone signed 64-bit key.  (Not site_table.hpp's unsigned table_key: they order a negative rname differently.)
__device__ __forceinline__ int64_t site_key(int32_t c, int32_t p) { return (int64_t)c * 4294967296LL + ((int64_t)p + 2147483648LL); }

// first i in [0, n) with key(chr[i], pos[i]) >= q, by the whole wavefront (uniform result): every step the 64 lanes probe
// 64 evenly spaced sites and the count of those below q narrows the range to one stride
__device__ inline int64_t wave_lower_bound(const int32_t *__restrict__ chr, const int32_t *__restrict__ pos, int64_t n, int64_t q) {
  const int lane = threadIdx.x & 63;
  int64_t a = 0, b = n;
  while (b > a) {
    const int64_t s = (b - a + 63) / 64;
    const int64_t p = a + (int64_t)lane * s;
    const bool less = p < b && site_key(chr[p], pos[p]) < q;
    const int c = __popcll(__ballot(less));
    if (c == 0) break;                               // site a is already >= q
    const int64_t next = a + (int64_t)c * s;
    a = a + (int64_t)(c - 1) * s + 1;
    b = next < b ? next : b;
  }
  return a;
}

// sequential lower bound over a sorted key array
__device__ __forceinline__ int32_t lds_lower_bound(const int64_t *k, int32_t n, int64_t q) {
  int32_t a = 0, b = n;
  while (a < b) { const int32_t m = (a + b) >> 1; if (k[m] < q) a = m + 1; else b = m; }
  return a;
}
__device__ __forceinline__ int64_t glb_lower_bound(const int32_t *chr, const int32_t *pos, int64_t a, int64_t b, int64_t q) {
  while (a < b) { const int64_t m = (a + b) >> 1; if (site_key(chr[m], pos[m]) < q) a = m + 1; else b = m; }
  return a;
}

// seq_nt16_int: A C G T (nt16 1 2 4 8) -> 0 1 2 3, every other code -> 4 (N), one nibble per code
constexpr uint64_t kNt16Int = 0x4444444344424104ULL;

}  // namespace epi
