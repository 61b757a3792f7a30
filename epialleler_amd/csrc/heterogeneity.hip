// Heterogeneity report: epiallele entropy, epipolymorphism and the fraction of discordant reads per window of k
// neighbouring sites (include/epihip.h, epi_batch_heterogeneity_report_dev, has the definitions).  No reference interface
// is replaced; the report composes two reference rules: the site table is rcpp_cx_report with an all-TRUE pass vector
// (src/rcpp_cx_report.cpp:58-80, the majority rule) and the rows that count are those the read rule of rcpp_mhl_report
// keeps (src/rcpp_mhl_report.cpp:172-179, hmin = 0).
//
// Data path, all on the report's stream:
//  (a) the per-strand site table, the read rule and a row's site range [lo, hi): shared with the other reports (site_table.hpp).
//  (b) k_het_count: a group of G lanes (16, or 64 for long rows) takes a row.  It reads the row once for the read rule,
//      finds its site range [lo, hi) by a (G + 1)-ary search, and walks it G sites at a time: every lane loads the one byte at
//      its site, two ballots give the group's valid and methylated masks, the lane of the LAST site of a window takes
//      the k bits that end at it (the previous round's last k - 1 bits carried over) and, when all k are valid, adds 1
//      to counts[first site of the window][pattern].  Windows never leave the row's (rname, strand): [lo, hi) does not.
//  (c) k_het_keep (a thread per CX row = per window start): n, min_reads, the span cap -> a flag; util.hip's scan turns
//      the flags into output rows (site_rows); k_het_emit (at fetch) writes het_metrics of the window's histogram into
//      the caller's columns.  The bin sums run over the bins in ascending order inside one thread: no launch shape
//      enters the result.
// The state all of this leaves on the batch is epi_batch::sites (SiteReportState, common.hpp).
//
// Contention.  Rows arrive sorted by (rname, start): on a deep amplicon the rows of a wave share their windows and mostly
// their pattern.  With 16-lane groups the four rows of a wave walk the same sites when they start together, so lane j
// of every group then holds the same counter: the lanes compare their counter index with the three lanes j + 16 m
// and the lowest of a set adds the set's size.  EPI_HET_PER_LANE (make timing-het) adds 1 per lane instead;
// profiles/heterogeneity_report.txt has both on the two workloads.
#include "het_common.hpp"

namespace epi {

constexpr int64_t kHetCountsCap = 4LL << 30;          // bytes of counters (nsites * 2^k * 4) a report may allocate

struct HetArgs : SiteRows {
  int32_t k;
  uint32_t *counts;                   // [N << k]
};

template <int G>
__global__ __launch_bounds__(SITE_WG) void k_het_count(HetArgs a) {
  constexpr int GPW = 64 / G;                                // groups per wave
  const uint32_t lane = threadIdx.x & 63u, sub = lane % G, grp = lane / G;
  const int64_t row = ((int64_t)blockIdx.x * (SITE_WG / 64) + (threadIdx.x >> 6)) * GPW + grp;
  const SiteRow<G> r(a, row, sub, grp);
  const uint32_t lo = r.lo, hi = r.hi;

  const int k = a.k;
  const uint32_t full = (1u << k) - 1u;
  unsigned long long carry_v = 0, carry_m = 0;               // the k - 1 sites in front of this round, oldest at bit 0
  for (uint32_t base = lo; __ballot(base < hi) != 0ull; base += G) {
    const uint32_t g = base + sub;
    bool valid, meth;
    r.call(a, g, valid, meth);
    const unsigned long long sv = group_ballot<G>(valid, grp), sm = group_ballot<G>(meth, grp);
    // the k sites that end at this lane's: from this round, and from the carry for the first k - 1 lanes
    const int back = k - 1;
    unsigned long long wv, wm;
    if ((int)sub >= back) { wv = sv >> (sub - back); wm = sm >> (sub - back); }
    else { wv = (sv << (back - sub)) | (carry_v >> sub); wm = (sm << (back - sub)) | (carry_m >> sub); }
    const bool covered = ((uint32_t)wv & full) == full && g < hi;
    const uint32_t idx = covered ? ((g - (uint32_t)back) << k) | ((uint32_t)wm & full) : 0xFFFFFFFFu;
#if defined(EPI_HET_PER_LANE)
    if (covered) atomicAdd(&a.counts[idx], 1u);
#else
    if (G < 64) {
      // rows of one wave that walk the same sites hold the same counter in lane `sub` of their groups
      uint32_t same = 1u;
      bool first = true;
#pragma unroll
      for (int m = 1; m < GPW; m++) {
        const uint32_t other = __shfl(idx, (int)((lane + m * G) & 63u), 64);
        const bool below = ((lane + m * G) & 63u) < lane;
        if (other == idx) { same++; if (below) first = false; }
      }
      if (covered && first) atomicAdd(&a.counts[idx], same);
    } else {
      if (covered) atomicAdd(&a.counts[idx], 1u);
    }
#endif
    carry_v = (sv >> (G - back)) & ((1ull << back) - 1ull);
    carry_m = (sm >> (G - back)) & ((1ull << back) - 1ull);
  }
}

__global__ __launch_bounds__(SITE_WG) void k_het_keep(HetFinish f, uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (i >= f.N) return;
  int32_t end = 0;
  const uint32_t *c = het_window(f, i, &end);
  uint32_t keep = 0;
  if (c) {
    uint64_t n = 0;
    for (int b = 0; b < (1 << f.k); b++) n += c[b];
    const int64_t span = (int64_t)end - (int64_t)f.pos[i] + 1;
    keep = n >= (uint64_t)f.min_reads && (f.max_span == 0 || span <= f.max_span) ? 1u : 0u;
  }
  flag[i] = keep;
}

struct HetOut {
  int32_t *rname, *strand, *pos, *end, *context, *nreads, *npatterns;
  double *beta, *epipoly, *entropy, *pdr;
  int32_t *counts;                    // [nrow][2^k] or null
};

__global__ __launch_bounds__(SITE_WG) void k_het_emit(HetFinish f, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ out_off,
                                                     HetOut o) {
  const uint32_t i = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (i >= f.N || !flag[i]) return;
  int32_t end = 0;
  const uint32_t *c = het_window(f, i, &end);
  if (!c) return;
  const uint32_t r = out_off[i];
  const HetMetrics m = het_metrics(c, f.k, o.counts ? o.counts + ((size_t)r << f.k) : nullptr);
  o.rname[r] = f.rname[i]; o.strand[r] = f.strand[i]; o.pos[r] = f.pos[i]; o.end[r] = end; o.context[r] = f.context[i];
  o.nreads[r] = (int32_t)m.n; o.npatterns[r] = m.npatterns;
  o.beta[r] = m.beta; o.epipoly[r] = m.epipoly; o.entropy[r] = m.entropy; o.pdr[r] = m.pdr;
}

void het_finish_args(const epi_batch *b, HetFinish &f) {
  f.N = site_view_args(b, f);
  f.k = b->sites.het.k;
  f.min_reads = b->sites.min_reads;
  f.max_span = b->sites.het.max_span;
}

int het_check_window(const char *who, int k, int32_t max_window_span) {
  if (k < kHetMinK || k > kHetMaxK) return fail(EPI_ERR_ARG, "%s: k = %d, windows hold %d to %d sites", who, k, kHetMinK, kHetMaxK);
  if (max_window_span < 0) return fail(EPI_ERR_ARG, "%s: negative max_window_span", who);
  return EPI_OK;
}

int64_t het_counter_bytes(int64_t nsites, int k) {
  if (nsites < 0 || k < kHetMinK || k > kHetMaxK || nsites >= (1LL << 31)) return -1;
  const int64_t bytes = (nsites << k) * 4;
  return bytes > kHetCountsCap ? -1 : bytes;
}

int het_count_launch(const SiteRows &rows, int k, uint32_t *counts, int64_t nb_rows, bool wide, hipStream_t s) {
  HetArgs a;
  static_cast<SiteRows &>(a) = rows;
  a.k = k;
  a.counts = counts;
  if (wide) hipLaunchKernelGGL((k_het_count<64>), dim3((unsigned)nb_rows), dim3(SITE_WG), 0, s, a);
  else hipLaunchKernelGGL((k_het_count<16>), dim3((unsigned)nb_rows), dim3(SITE_WG), 0, s, a);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

static int het_report(epi_batch *b, const char *ctx, int k, double max_oo, int32_t min_reads, int32_t max_span, hipStream_t s,
                      int64_t *nrow_out) {
  SiteReportState &t = b->sites;
  // (a) the site table
  int64_t nsite = 0;
  EPI_TRY(site_cx_report(b, ctx, s, "epi_batch_heterogeneity_report_dev", &nsite));
  t.nsite = nsite; t.het.k = k;
  t.min_reads = (uint32_t)(min_reads > 1 ? min_reads : 1);
  t.het.max_span = max_span;
  if (nsite < k) { b->last_kind = KIND_HET; b->last_nrow = 0; t.nsite = 0; return EPI_OK; }
  if (het_counter_bytes(nsite, k) < 0)
    return fail(EPI_ERR_ARG, "epi_batch_heterogeneity_report_dev: %lld sites x %d patterns need %lld bytes of counters, above the cap of %lld",
                (long long)nsite, 1 << k, (long long)((nsite << k) * 4), (long long)kHetCountsCap);
  const size_t N = (size_t)nsite;
  const int64_t nb_sites = ((int64_t)N + SITE_WG - 1) / SITE_WG;
  bool wide = false;
  const int64_t nb_rows = site_count_blocks(b, &wide);
  EPI_TRY(check_grid(nb_rows, SITE_WG, "heterogeneity counting kernel"));
  EPI_TRY(site_table(b, nsite, s));
  EPI_TRY(t.counts.ensure((N << k) * 4));
  uint32_t *flag = t.flag.as<uint32_t>();

  // (b) the histograms
  EPI_HIP(hipMemsetAsync(t.counts.p, 0, (N << k) * 4, s));
  SiteRows a;
  site_rows_args(b, ctx_mask_of(ctx), max_oo, a);
  prof_begin("het_count", s);
  const int rc_count = het_count_launch(a, k, t.counts.as<uint32_t>(), nb_rows, wide, s);
  prof_end("het_count", s);
  EPI_TRY(rc_count);

  // (c) which windows are reported, and where
  HetFinish f;
  het_finish_args(b, f);
  hipLaunchKernelGGL(k_het_keep, dim3((unsigned)nb_sites), dim3(SITE_WG), 0, s, f, flag);
  EPI_HIP(hipGetLastError());
  EPI_TRY(t.out.ensure(N * 4));
  EPI_TRY(site_rows(b, flag, (int64_t)N, t.out.as<uint32_t>(), &t.scalars()->nrow, s, nrow_out));
  b->last_kind = KIND_HET;
  b->last_nrow = *nrow_out;
  return EPI_OK;
}

}  // namespace epi

using namespace epi;

extern "C" {

int epi_heterogeneity_counter_bytes(int64_t nsites, int k, int64_t *bytes_out) {
  if (!bytes_out) return fail(EPI_ERR_ARG, "epi_heterogeneity_counter_bytes: NULL argument");
  *bytes_out = 0;
  if (nsites < 0 || k < kHetMinK || k > kHetMaxK)
    return fail(EPI_ERR_ARG, "epi_heterogeneity_counter_bytes: %lld sites, k = %d (%d to %d)", (long long)nsites, k, kHetMinK, kHetMaxK);
  const int64_t bytes = het_counter_bytes(nsites, k);
  if (bytes < 0)
    return fail(EPI_ERR_ARG, "epi_heterogeneity_counter_bytes: %lld sites x %d patterns need more than %lld bytes of counters",
                (long long)nsites, 1 << k, (long long)kHetCountsCap);
  *bytes_out = bytes;
  return EPI_OK;
}

int epi_batch_heterogeneity_report_dev(epi_batch *b, const char *ctx, int k, double max_ooctx_meth_frac, int32_t min_reads,
                                       int32_t max_window_span, void *stream, int64_t *nrow_out) {
  if (!b || !ctx || !nrow_out) return fail(EPI_ERR_ARG, "epi_batch_heterogeneity_report_dev: NULL argument");
  *nrow_out = 0;
  EPI_TRY(het_check_window("epi_batch_heterogeneity_report_dev", k, max_window_span));
  b->last_kind = KIND_NONE;
  EPI_HIP(hipSetDevice(b->eng->device));
  return het_report(b, ctx, k, max_ooctx_meth_frac, min_reads, max_window_span, pick_stream(b, stream), nrow_out);
}

int epi_batch_heterogeneity_fetch_dev(epi_batch *b, int32_t *const d_icols[7], double *const d_dcols[4], int32_t *d_counts,
                                      void *stream) {
  hipStream_t s = nullptr;
  int64_t nrow = 0;
  EPI_TRY(site_fetch_begin("epi_batch_heterogeneity_fetch_dev", b, KIND_HET, "heterogeneity report", false, d_icols, 7, d_dcols, 4, stream, &s, &nrow));
  if (nrow == 0) return EPI_OK;
  HetFinish f;
  het_finish_args(b, f);
  HetOut o;
  o.rname = d_icols[0]; o.strand = d_icols[1]; o.pos = d_icols[2]; o.end = d_icols[3]; o.context = d_icols[4];
  o.nreads = d_icols[5]; o.npatterns = d_icols[6];
  o.beta = d_dcols[0]; o.epipoly = d_dcols[1]; o.entropy = d_dcols[2]; o.pdr = d_dcols[3];
  o.counts = d_counts;
  const unsigned nb = (unsigned)(((int64_t)f.N + SITE_WG - 1) / SITE_WG);
  prof_begin("het_emit", s);
  hipLaunchKernelGGL(k_het_emit, dim3(nb), dim3(SITE_WG), 0, s, f, b->sites.flag.as<uint32_t>(), b->sites.out.as<uint32_t>(), o);
  prof_end("het_emit", s);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

}  // extern "C"
