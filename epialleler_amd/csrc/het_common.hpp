// What the heterogeneity report (heterogeneity.hip), the linkage report (linkage.hip) and the heterogeneity comparison
// (het_compare.hip) share: the per-strand site table of the batch's un-thresholded CX report, the read rule, a row's site
// range in that table and its call at a site.  All count on the same data path (heterogeneity.hip has its description);
// the reports differ in what a row adds to, the comparison counts two batches with the heterogeneity report's kernel on
// the sites both have.
#pragma once
#include "common.hpp"
#include <string.h>

namespace epi {

constexpr int HET_WG = 256;
constexpr int64_t kHetLongRow = 512;                  // mean row bytes above which a whole wave takes a row

// The rows of the batch and the site table, as a counting kernel sees them
struct HetRows {
  const uint8_t *xm;
  const int64_t *off;
  const int32_t *len, *rname, *strand, *start;
  int64_t n;
  const unsigned long long *key;      // [N] per-strand site table
  const uint8_t *sctx;                // [N] context code of the site (2 CHH, 6 CHG, 7 CG)
  const uint32_t *n1;                 // '+' sites
  uint32_t N;
  uint32_t oom_mask, oou_mask;        // out-of-context methylated / unmethylated nibble codes (those not in the context)
  double max_oo;
};

__device__ __forceinline__ unsigned long long het_key(int32_t rname, int64_t pos) {
  return ((unsigned long long)(uint32_t)rname << 32) + (unsigned long long)(pos + kPosBias);
}
__device__ __forceinline__ int32_t het_key_pos(unsigned long long key) {
  return (int32_t)(uint32_t)((key & 0xFFFFFFFFull) - (unsigned long long)kPosBias);
}

// First index in [a, b) whose key is >= key, searched by the G lanes of a group at once: the lanes probe G evenly spaced
// entries, the ballot of "below the key" (ones, then zeros: the table is sorted) picks one of the G + 1 parts, and a part of
// at most G entries is probed whole.  log_{G+1} dependent loads instead of log_2: 6 instead of 22 for 3.5 M sites and 16
// lanes, and the loads are what the kernel waits for.  Every lane of the wave calls this together; the lanes of a group pass
// the same a, b and key (a = b: nothing to search).
template <int G>
__device__ __forceinline__ uint32_t het_lower_bound(const unsigned long long *__restrict__ keys, uint32_t a, uint32_t b,
                                                    unsigned long long key, uint32_t sub, uint32_t grp) {
  const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << (G % 64)) - 1ull);
  while (__ballot(a < b) != 0ull) {
    const uint32_t span = b - a;
    const bool last = span <= (uint32_t)G;
    const uint32_t m = last ? a + sub : a + (uint32_t)(((uint64_t)span * (sub + 1u)) / (uint32_t)(G + 1));
    const bool below = m < b && keys[m] < key;
    const uint32_t cnt = (uint32_t)__popcll((__ballot(below) >> (grp * G)) & gmask);
    if (last) {
      a = b = a + cnt;
    } else {
      const uint32_t na = cnt > 0u ? a + (uint32_t)(((uint64_t)span * cnt) / (uint32_t)(G + 1)) + 1u : a;
      const uint32_t nb = cnt < (uint32_t)G ? a + (uint32_t)(((uint64_t)span * (cnt + 1u)) / (uint32_t)(G + 1)) : b;
      a = na; b = nb;
    }
  }
  return a;
}

// ordinal of CX row i in the per-strand table (rank: '+' rows in front of it)
__device__ __forceinline__ uint32_t het_ordinal(int32_t strand, uint32_t i, uint32_t rank, uint32_t n1) {
  return strand == 1 ? rank : n1 + (i - rank);
}

// What a group of G lanes (lane `sub` of group `grp` of its wave) learns of its row before it counts: the row's bytes and
// start, and its sites [lo, hi) of its strand's part of the table -- empty when the read rule drops the row.
template <int G>
struct HetRow {
  const uint8_t *p;
  int32_t start;
  uint32_t lo, hi;

  __device__ __forceinline__ HetRow(const HetRows &a, int64_t row, uint32_t sub, uint32_t grp) {
    const bool have = row < a.n;
    const int32_t st = have ? a.strand[row] : 0;
    const int32_t len = have && (st == 1 || st == 2) ? a.len[row] : 0;
    const int64_t off = have ? a.off[row] : 0;
    start = have ? a.start[row] : 0;
    p = a.xm + off;

    // the read rule (rcpp_mhl_report.cpp:172-179, hmin = 0): four bytes per lane and step
    uint32_t om = 0, ou = 0;
    for (int32_t c = (int32_t)sub * 4; c < len; c += G * 4) {
      uint32_t w = 0x0C0C0C0Cu;                                // '.': in neither class
      if (c + 4 <= len) memcpy(&w, p + c, 4);
      else for (int32_t j = 0; c + j < len; j++) w = (w & ~(0xFFu << (8 * j))) | ((uint32_t)p[c + j] << (8 * j));
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t nib = (w >> (8 * j)) & 15u;
        om += (a.oom_mask >> nib) & 1u;
        ou += (a.oou_mask >> nib) & 1u;
      }
    }
#pragma unroll
    for (int d = 1; d < G; d <<= 1) { om += __shfl_xor(om, d, 64); ou += __shfl_xor(ou, d, 64); }
    const double frac = (double)om / (double)((uint64_t)om + ou);       // :178 (0 / 0 = NaN: kept)
    const bool keep = len > 0 && !(frac > a.max_oo);

    // the row's sites: [lo, hi) of its strand's part of the table
    const uint32_t n1 = *a.n1;
    const uint32_t s0 = st == 1 ? 0u : n1, s1 = st == 1 ? n1 : a.N;
    const int32_t rn = keep ? a.rname[row] : 0;
    lo = het_lower_bound<G>(a.key, keep ? s0 : 0u, keep ? s1 : 0u, het_key(rn, (int64_t)start), sub, grp);
    const uint32_t cap = (uint64_t)lo + (uint32_t)len < s1 ? lo + (uint32_t)len : s1;   // at most one site per position
    hi = het_lower_bound<G>(a.key, keep ? lo : 0u, keep ? cap : 0u, het_key(rn, (int64_t)start + len), sub, grp);
  }

  // the row's call at site g of the table: none for g >= hi
  __device__ __forceinline__ void call(const HetRows &a, uint32_t g, bool &valid, bool &meth) const {
    valid = false; meth = false;
    if (g < hi) {
      const int32_t pos = het_key_pos(a.key[g]);
      const uint32_t nib = p[pos - start] & 15u;               // start <= pos < start + len: the search's bounds
      valid = (nib & 7u) == a.sctx[g];
      meth = valid && nib < 8u;
    }
  }
};

// What the kernels behind the counting see (heterogeneity.hip, het_compare.hip): the site table in CX row order, the
// per-strand table and the counters of the windows
struct HetFinish {
  const int32_t *rname, *strand, *pos, *context;   // the CX table
  const uint32_t *rank, *n1;
  const unsigned long long *key;
  const uint32_t *counts;
  uint32_t N;
  int32_t k;
  uint32_t min_reads;
  int64_t max_span;
};

// the window that starts at CX row i: its counters, or null when fewer than k sites follow on its (rname, strand)
__device__ __forceinline__ const uint32_t *het_window(const HetFinish &f, uint32_t i, int32_t *end) {
  const int32_t st = f.strand[i];
  const uint32_t n1 = *f.n1;
  const uint32_t g = het_ordinal(st, i, f.rank[i], n1), seg_end = st == 1 ? n1 : f.N;
  const uint32_t last = g + (uint32_t)f.k - 1u;
  if (last >= seg_end) return nullptr;
  const unsigned long long kl = f.key[last];
  if ((uint32_t)(kl >> 32) != (uint32_t)f.rname[i]) return nullptr;
  *end = het_key_pos(kl);
  return f.counts + ((size_t)g << f.k);
}

constexpr int kHetMinK = 2, kHetMaxK = 6;
// bytes of counters (nsites * 2^k * 4) of a heterogeneity report or of one side of a comparison, or -1 when a report
// refuses them: above 4 GiB, or sites beyond 32-bit ordinals
int64_t het_counter_bytes(int64_t nsites, int k);

// Host side (heterogeneity.hip).  het_cx_sites: the un-thresholded CX report of the upper-case letters of ctx, as
// epi_batch_cx_report_dev(b, NULL, those) runs it; refuses a batch set up for a sharded report (`who` names the caller in
// the message) and leaves last_kind = KIND_NONE.  het_site_table: that report's six columns fetched into het_cx, every
// row's '+' rank in het_rank, the per-strand table in het_key / het_sctx and the '+' site count in het_scal[0]
// (het_scal[1] is the caller's); nsite >= 1.  het_flag holds nsite scratch words afterwards.  Its two halves on their
// own: het_cx_fetch brings the six columns into `cx` ([6][nsite]), het_strand_table makes rank, key, context and '+'
// count from a table of nsite rows that is in het_cx already (its first four columns, [.][nsite]).
int het_cx_sites(epi_batch *b, const char *ctx, hipStream_t s, const char *who, int64_t *nsite);
int het_cx_fetch(epi_batch *b, int64_t nsite, hipStream_t s, DevBuf &cx);
int het_strand_table(epi_batch *b, int64_t nsite, hipStream_t s);
int het_site_table(epi_batch *b, int64_t nsite, hipStream_t s);
// the rows, the table and the read rule's masks for the contexts of ctx_mask
void het_rows_args(const epi_batch *b, uint32_t ctx_mask, double max_oo, HetRows &a);
// the site table, window size, thresholds and counters (het_counts) of the last report on b
void het_finish_args(const epi_batch *b, HetFinish &f);
// k_het_count<16> or <64> (heterogeneity.hip): the rows of `a` add to counts [a.N << k], which the caller has zeroed;
// nb_rows and wide are het_count_blocks' of the batch the rows are of
int het_count_launch(const HetRows &a, int k, uint32_t *counts, int64_t nb_rows, bool wide, hipStream_t s);
// workgroups of a counting kernel, and whether a whole wave takes a row
inline int64_t het_count_blocks(const epi_batch *b, bool *wide) {
  *wide = b->nbytes > kHetLongRow * b->n;
  const int rows = *wide ? HET_WG / 64 : HET_WG / 16;
  return (b->n + rows - 1) / rows;
}

}  // namespace epi
