// The per-strand site table of a batch's un-thresholded CX report, which the heterogeneity, linkage, heterogeneity comparison
// and FDRP reports count over: its construction (site_table.hip), a row's site range in it under the read rule and the row's
// call at a site, the device view that the kernels behind the counting take, the step from keep flags to output rows and what
// a fetch does first.  The table and what the last report left are kept in epi_batch::sites (SiteReportState, common.hpp).
// Data path, on the report's stream: the un-thresholded CX report of the batch is fetched into sites.cx (six columns of N
// rows, in (rname, pos, strand) order).  A scan over "strand is +" gives every row its ordinal in a table split per
// strand: '+' sites at [0, n1), '-' sites at [n1, N), each sorted by (rname, pos).  k_site_keys writes that table: a 64-bit
// key (rname << 32) + (pos + 2^31) to search in, and the site's context code.  SiteRow is a row's walk into it.
#pragma once
#include "common.hpp"
#include <string.h>

namespace epi {

constexpr int SITE_WG = 256;
constexpr int64_t kSiteLongRow = 512;                 // mean row bytes above which a whole wave takes a row

// The rows of the batch and the site table, as a counting kernel sees them
struct SiteRows {
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

// The table's search key: unsigned, rname in the upper half.  (Not site_search.hpp's signed site_key: they order a negative rname differently.)
__device__ __forceinline__ unsigned long long table_key(int32_t rname, int64_t pos) {
  return ((unsigned long long)(uint32_t)rname << 32) + (unsigned long long)(pos + kPosBias);
}
__device__ __forceinline__ int32_t table_key_pos(unsigned long long key) {
  return (int32_t)(uint32_t)((key & 0xFFFFFFFFull) - (unsigned long long)kPosBias);
}

// the bits of group `grp` (G lanes) in the wave's ballot of pred (an int, as __ballot takes it), lane `sub` at bit `sub`
template <int G>
__device__ __forceinline__ unsigned long long group_ballot(int pred, uint32_t grp) {
  const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << (G % 64)) - 1ull);
  return (__ballot(pred) >> (grp * G)) & gmask;
}

// First index in [a, b) whose key is >= key, searched by the G lanes of a group at once: the lanes probe G evenly spaced
// entries, the ballot of "below the key" (ones, then zeros: the table is sorted) picks one of the G + 1 parts, and a part of
// at most G entries is probed whole.  log_{G+1} dependent loads instead of log_2: 6 instead of 22 for 3.5 M sites and 16
// lanes, and the loads are what the kernel waits for.  Every lane of the wave calls this together; the lanes of a group pass
// the same a, b and key (a = b: nothing to search).
template <int G>
__device__ __forceinline__ uint32_t site_lower_bound(const unsigned long long *__restrict__ keys, uint32_t a, uint32_t b,
                                                     unsigned long long key, uint32_t sub, uint32_t grp) {
  while (__ballot(a < b) != 0ull) {
    const uint32_t span = b - a;
    const bool last = span <= (uint32_t)G;
    const uint32_t m = last ? a + sub : a + (uint32_t)(((uint64_t)span * (sub + 1u)) / (uint32_t)(G + 1));
    const bool below = m < b && keys[m] < key;
    const uint32_t cnt = (uint32_t)__popcll(group_ballot<G>(below, grp));
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
__device__ __forceinline__ uint32_t site_ordinal(int32_t strand, uint32_t i, uint32_t rank, uint32_t n1) {
  return strand == 1 ? rank : n1 + (i - rank);
}

// What a group of G lanes (lane `sub` of group `grp` of its wave) learns of its row before it counts: the row's bytes and
// start, and its sites [lo, hi) of its strand's part of the table -- empty when the read rule drops the row.
template <int G>
struct SiteRow {
  const uint8_t *p;
  int32_t start;
  uint32_t lo, hi;

  __device__ __forceinline__ SiteRow(const SiteRows &a, int64_t row, uint32_t sub, uint32_t grp) {
    const bool have = row < a.n;
    const int32_t st = have ? a.strand[row] : 0;
    const int32_t len = have && (st == 1 || st == 2) ? a.len[row] : 0;
    const int64_t off = have ? a.off[row] : 0;
    start = have ? a.start[row] : 0;
    p = a.xm + off;

    // the read rule's counts (rcpp_mhl_report.cpp:172-179, hmin = 0): four bytes per lane and step
    uint32_t om = 0, ou = 0;
    for (int32_t c = (int32_t)sub * 4; c < len; c += G * 4) {
      uint32_t w = kXmDot4;                                    // '.': in neither class
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
    const bool keep = read_rule_keeps(len, om, ou, a.max_oo);

    // the row's sites: [lo, hi) of its strand's part of the table
    const uint32_t n1 = *a.n1;
    const uint32_t s0 = st == 1 ? 0u : n1, s1 = st == 1 ? n1 : a.N;
    const int32_t rn = keep ? a.rname[row] : 0;
    lo = site_lower_bound<G>(a.key, keep ? s0 : 0u, keep ? s1 : 0u, table_key(rn, (int64_t)start), sub, grp);
    const uint32_t cap = (uint64_t)lo + (uint32_t)len < s1 ? lo + (uint32_t)len : s1;   // at most one site per position
    hi = site_lower_bound<G>(a.key, keep ? lo : 0u, keep ? cap : 0u, table_key(rn, (int64_t)start + len), sub, grp);
  }

  // the row's call at site g of the table: none for g >= hi
  __device__ __forceinline__ void call(const SiteRows &a, uint32_t g, bool &valid, bool &meth) const {
    valid = false; meth = false;
    if (g < hi) {
      const int32_t pos = table_key_pos(a.key[g]);
      const uint32_t nib = p[pos - start] & 15u;               // start <= pos < start + len: the search's bounds
      valid = (nib & 7u) == a.sctx[g];
      meth = valid && nib < 8u;
    }
  }
};

// The site table as the kernels behind the counting see it: in CX row order, split per strand, and the counters over it.
// (Its row count N is the first member of the structs that derive from it: a 32-bit member at the end of this one would
// move what follows it in their kernel arguments by the padding behind it.)
struct SiteView {
  const int32_t *rname, *strand, *pos, *context;   // the CX table
  const uint32_t *rank, *n1;
  const unsigned long long *key;
  const uint32_t *counts;
};

// Host side (site_table.hip); `sites` is epi_batch::sites.  site_cx_report: the un-thresholded CX report of the upper-case
// letters of ctx, as epi_batch_cx_report_dev(b, NULL, those) runs it; refuses a batch set up for a sharded report (`who`
// names the caller) and leaves last_kind = KIND_NONE.  site_table (nsite >= 1): that report's six columns into sites.cx
// (site_cx_fetch, [6][nsite]), then from a table that is in sites.cx (site_strand_table) every row's '+' rank in sites.rank,
// the per-strand table in sites.key / sites.sctx and the '+' site count in the scalar nplus; sites.flag is its scratch.
int site_cx_report(epi_batch *b, const char *ctx, hipStream_t s, const char *who, int64_t *nsite);
int site_cx_fetch(epi_batch *b, int64_t nsite, hipStream_t s, DevBuf &cx);
int site_strand_table(epi_batch *b, int64_t nsite, hipStream_t s);
int site_table(epi_batch *b, int64_t nsite, hipStream_t s);
// the rows, the table and the read rule's masks for the contexts of ctx_mask
void site_rows_args(const epi_batch *b, uint32_t ctx_mask, double max_oo, SiteRows &a);
// the site table of b and its counters; returns its rows (sites.nsite)
uint32_t site_view_args(const epi_batch *b, SiteView &v);
// Which rows are reported, and where: the exclusive scan of the n keep flags into off, their total into `total` (a field
// of b's SiteScalars) and from there to the host -- the step's one synchronisation.  A profiling range `prof` that the
// caller has open around its keep kernel ends behind the scan.
int site_rows(epi_batch *b, const uint32_t *flag, int64_t n, uint32_t *off, uint32_t *total, hipStream_t s, int64_t *count,
              const char *prof = nullptr);
// What a fetch entry point `who` does first: its arguments, the finished report on b (`kind`; `what` names it in the
// message; blocks: those of the linkage report), the ni + nd columns, the device and the stream.  *nrow = 0: nothing to write.
int site_fetch_begin(const char *who, epi_batch *b, ReportKind kind, const char *what, bool blocks, int32_t *const *icols, int ni,
                     double *const *dcols, int nd, void *stream, hipStream_t *s, int64_t *nrow);
// workgroups of a kernel whose groups take a row each, and whether a whole wave takes a row
inline int64_t site_count_blocks(const epi_batch *b, bool *wide) {
  *wide = b->nbytes > kSiteLongRow * b->n;
  const int rows = *wide ? SITE_WG / 64 : SITE_WG / 16;
  return (b->n + rows - 1) / rows;
}

}  // namespace epi
