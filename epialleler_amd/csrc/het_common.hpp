// What the heterogeneity report (heterogeneity.hip), the linkage report (linkage.hip) and the heterogeneity comparison
// (het_compare.hip) share: the per-strand site table of the batch's un-thresholded CX report, the read rule, a row's site
// range in that table and its call at a site; the device view of the table that the kernels behind the counting take, the
// step from keep flags to output rows, the per-sample metrics of a histogram and the checks of the entry points.  All
// count on the same data path (heterogeneity.hip has its description) and keep their state in one place, epi_batch::sites
// (SiteReportState, common.hpp); the reports differ in what a row adds to, the comparison counts two batches with the
// heterogeneity report's kernel on the sites both have.
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
// the bits of group `grp` (G lanes) in the wave's ballot of pred, lane `sub` of the group at bit `sub` (pred: an int, as
// __ballot takes it)
template <int G>
__device__ __forceinline__ unsigned long long group_ballot(int pred, uint32_t grp) {
  const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << (G % 64)) - 1ull);
  return (__ballot(pred) >> (grp * G)) & gmask;
}

template <int G>
__device__ __forceinline__ uint32_t het_lower_bound(const unsigned long long *__restrict__ keys, uint32_t a, uint32_t b,
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

// The site table as the kernels behind the counting see it: in CX row order, split per strand, and the counters over it.
// (Its row count N is the first member of the structs that derive from it: a 32-bit member at the end of this one would
// move what follows it in their kernel arguments by the padding behind it.)
struct SiteView {
  const int32_t *rname, *strand, *pos, *context;   // the CX table
  const uint32_t *rank, *n1;
  const unsigned long long *key;
  const uint32_t *counts;
};

// ... with the windows of a heterogeneity report or a comparison (heterogeneity.hip, het_compare.hip)
struct HetFinish : SiteView {
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

// What one histogram c[2^k] says of its sample.  The bin sums run over the bins in ascending order inside one thread; hist,
// when given, receives the histogram as a row of int32.
struct HetMetrics {
  uint64_t n;
  int32_t npatterns;
  double beta, epipoly, entropy, pdr;
};
__device__ __forceinline__ HetMetrics het_metrics(const uint32_t *c, int k, int32_t *hist) {
  const int nb = 1 << k;
  uint64_t n = 0, nmeth = 0;
  int32_t npat = 0;
  for (int b = 0; b < nb; b++) { const uint32_t v = c[b]; n += v; nmeth += (uint64_t)v * (uint32_t)__popc(b); npat += v ? 1 : 0; }
  const double dn = (double)n;
  double sq = 0.0, ent = 0.0;
  for (int b = 0; b < nb; b++) {                              // ascending bins
    const uint32_t v = c[b];
    if (hist) hist[b] = (int32_t)v;
    if (!v) continue;
    const double pb = (double)v / dn;
    sq += pb * pb;
    ent += pb * log2(pb);
  }
  HetMetrics m;
  m.n = n; m.npatterns = npat;
  m.beta = (double)nmeth / (dn * (double)k);
  m.epipoly = 1.0 - sq;
  m.entropy = -ent / (double)k;
  m.pdr = 1.0 - (double)((uint64_t)c[0] + c[nb - 1]) / dn;
  return m;
}

constexpr int kHetMinK = 2, kHetMaxK = 6;
// bytes of counters (nsites * 2^k * 4) of a heterogeneity report or of one side of a comparison, or -1 when a report
// refuses them: above 4 GiB, or sites beyond 32-bit ordinals
int64_t het_counter_bytes(int64_t nsites, int k);

// Host side (heterogeneity.hip); `sites` is epi_batch::sites.  het_cx_sites: the un-thresholded CX report of the upper-case
// letters of ctx, as epi_batch_cx_report_dev(b, NULL, those) runs it; refuses a batch set up for a sharded report (`who`
// names the caller in the message) and leaves last_kind = KIND_NONE.  het_site_table: that report's six columns fetched
// into sites.cx, every row's '+' rank in sites.rank, the per-strand table in sites.key / sites.sctx and the '+' site count
// in the scalar nplus; nsite >= 1.  sites.flag holds nsite scratch words afterwards.  Its two halves on their own:
// het_cx_fetch brings the six columns into `cx` ([6][nsite]), het_strand_table makes rank, key, context and '+' count from
// a table of nsite rows that is in sites.cx already (its first four columns, [.][nsite]).
int het_cx_sites(epi_batch *b, const char *ctx, hipStream_t s, const char *who, int64_t *nsite);
int het_cx_fetch(epi_batch *b, int64_t nsite, hipStream_t s, DevBuf &cx);
int het_strand_table(epi_batch *b, int64_t nsite, hipStream_t s);
int het_site_table(epi_batch *b, int64_t nsite, hipStream_t s);
// the rows, the table and the read rule's masks for the contexts of ctx_mask
void het_rows_args(const epi_batch *b, uint32_t ctx_mask, double max_oo, HetRows &a);
// the site table of b and its counters; returns its rows (sites.nsite)
uint32_t site_view_args(const epi_batch *b, SiteView &v);
// ... with window size and thresholds of the last report on b
void het_finish_args(const epi_batch *b, HetFinish &f);
// Which rows are reported, and where: the exclusive scan of the n keep flags into off, their total into `total` (a field
// of b's SiteScalars) and from there to the host -- the step's one synchronisation.  A profiling range `prof` that the
// caller has open around its keep kernel ends behind the scan.
int site_rows(epi_batch *b, const uint32_t *flag, int64_t n, uint32_t *off, uint32_t *total, hipStream_t s, int64_t *count,
              const char *prof = nullptr);
// k and max_window_span as a report and a comparison take them (`who`: the entry point, for the message)
int het_check_window(const char *who, int k, int32_t max_window_span);
// What a fetch entry point `who` does first: its arguments, the report on b (`kind`; blocks: those of the linkage report),
// the ni + nd columns, the device and the stream.  *nrow = 0: nothing to write.
int site_fetch_begin(const char *who, epi_batch *b, ReportKind kind, bool blocks, int32_t *const *icols, int ni, double *const *dcols,
                     int nd, void *stream, hipStream_t *s, int64_t *nrow);
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
