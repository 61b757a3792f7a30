// Heterogeneity report: epiallele entropy, epipolymorphism and the fraction of discordant reads per window of k
// neighbouring sites (include/epihip.h, epi_batch_heterogeneity_report_dev, has the definitions).  No reference interface
// is replaced; the report composes two reference rules: the site table is rcpp_cx_report with an all-TRUE pass vector
// (src/rcpp_cx_report.cpp:58-80, the majority rule) and the rows that count are those the read rule of rcpp_mhl_report
// keeps (src/rcpp_mhl_report.cpp:172-179, hmin = 0).
//
// Data path, all on the report's stream:
// The site table, the read rule and a row's walk over its sites are shared with the linkage report (het_common.hpp).
//  (a) the un-thresholded CX report of the batch, fetched into sites.cx (six columns of N rows, in (rname, pos, strand)
//      order).  A scan over "strand is +" gives every row its ordinal in a table split per strand: '+' sites at
//      [0, n1), '-' sites at [n1, N), each sorted by (rname, pos).  k_het_sites writes that table: a 64-bit key
//      (rname << 32) + (pos + 2^31) to search in, and the site's context code.
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

struct HetArgs : HetRows {
  int32_t k;
  uint32_t *counts;                   // [N << k]
};

__global__ __launch_bounds__(HET_WG) void k_het_strand_flag(const int32_t *__restrict__ strand, uint32_t N, uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * (uint32_t)HET_WG + threadIdx.x;
  if (i < N) flag[i] = strand[i] == 1 ? 1u : 0u;
}

__global__ __launch_bounds__(HET_WG) void k_het_sites(const int32_t *__restrict__ rname, const int32_t *__restrict__ strand,
                                                      const int32_t *__restrict__ pos, const int32_t *__restrict__ context,
                                                      const uint32_t *__restrict__ rank, const uint32_t *__restrict__ n1p, uint32_t N,
                                                      unsigned long long *__restrict__ key, uint8_t *__restrict__ sctx) {
  const uint32_t i = blockIdx.x * (uint32_t)HET_WG + threadIdx.x;
  if (i >= N) return;
  const uint32_t g = het_ordinal(strand[i], i, rank[i], *n1p);
  if (g >= N) return;
  key[g] = het_key(rname[i], pos[i]);
  sctx[g] = (uint8_t)context[i];
}

template <int G>
__global__ __launch_bounds__(HET_WG) void k_het_count(HetArgs a) {
  constexpr int GPW = 64 / G;                                // groups per wave
  const uint32_t lane = threadIdx.x & 63u, sub = lane % G, grp = lane / G;
  const int64_t row = ((int64_t)blockIdx.x * (HET_WG / 64) + (threadIdx.x >> 6)) * GPW + grp;
  const HetRow<G> r(a, row, sub, grp);
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

__global__ __launch_bounds__(HET_WG) void k_het_keep(HetFinish f, uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * (uint32_t)HET_WG + threadIdx.x;
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

__global__ __launch_bounds__(HET_WG) void k_het_emit(HetFinish f, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ out_off,
                                                     HetOut o) {
  const uint32_t i = blockIdx.x * (uint32_t)HET_WG + threadIdx.x;
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

uint32_t site_view_args(const epi_batch *b, SiteView &v) {
  const SiteReportState &t = b->sites;
  const int32_t *cx = t.cx.as<int32_t>();
  const size_t N = (size_t)t.nsite;
  v.rname = cx; v.strand = cx + N; v.pos = cx + 2 * N; v.context = cx + 3 * N;
  v.rank = t.rank.as<uint32_t>();
  v.n1 = &t.scalars()->nplus;
  v.key = t.key.as<unsigned long long>();
  v.counts = t.counts.as<uint32_t>();
  return (uint32_t)N;
}

void het_finish_args(const epi_batch *b, HetFinish &f) {
  f.N = site_view_args(b, f);
  f.k = b->sites.k;
  f.min_reads = b->sites.min_reads;
  f.max_span = b->sites.max_span;
}

int site_rows(epi_batch *b, const uint32_t *flag, int64_t n, uint32_t *off, uint32_t *total, hipStream_t s, int64_t *count,
              const char *prof) {
  const int rc = scan_exclusive_u32(flag, off, n, total, b->scan_tmp, s);
  if (prof) prof_end(prof, s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(rc);
  // (the reported rows come back with the '+' count in front of them, 8 bytes; blocks and common sites alone, 4)
  SiteScalars *sc = b->sites.scalars();
  const uint32_t *first = total == &sc->nrow ? &sc->nplus : total;
  uint32_t h[2] = {0, 0};
  EPI_TRY(read_scalars(b, s, first, (size_t)(total - first + 1) * 4, h));
  *count = h[total - first];
  return EPI_OK;
}

int het_check_window(const char *who, int k, int32_t max_window_span) {
  if (k < kHetMinK || k > kHetMaxK) return fail(EPI_ERR_ARG, "%s: k = %d, windows hold %d to %d sites", who, k, kHetMinK, kHetMaxK);
  if (max_window_span < 0) return fail(EPI_ERR_ARG, "%s: negative max_window_span", who);
  return EPI_OK;
}

int site_fetch_begin(const char *who, epi_batch *b, ReportKind kind, bool blocks, int32_t *const *icols, int ni, double *const *dcols,
                     int nd, void *stream, hipStream_t *s, int64_t *nrow) {
  *nrow = 0;
  if (!b || !icols || !dcols) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  const char *what = blocks ? "epi_batch_linkage_blocks_dev" : kind == KIND_HET ? "heterogeneity report" : kind == KIND_LINK ? "linkage report"
                                                                                     : kind == KIND_FDRP ? "FDRP report" : "heterogeneity comparison";
  if (b->last_kind != kind || (blocks && !b->sites.blocks)) return fail(EPI_ERR_STATE, "%s: no finished %s on this batch", who, what);
  const int64_t n = blocks ? b->sites.nblock : b->last_nrow;
  if (n == 0) return EPI_OK;
  for (int i = 0; i < ni; i++) if (!icols[i]) return fail(EPI_ERR_ARG, "%s: NULL column", who);
  for (int i = 0; i < nd; i++) if (!dcols[i]) return fail(EPI_ERR_ARG, "%s: NULL column", who);
  EPI_HIP(hipSetDevice(b->eng->device));
  *s = pick_stream(b, stream);
  *nrow = n;
  return EPI_OK;
}

int het_cx_sites(epi_batch *b, const char *ctx, hipStream_t s, const char *who, int64_t *nsite) {
  // the un-thresholded CX report of the reported context(s), methylated letters only as in generateCytosineReport (the
  // table has a row per position whose majority is one of them, either case)
  char rep_ctx[8];
  int nrep = 0;
  const uint32_t ctx_mask = ctx_mask_of(ctx);
  for (const char *c = "HXZ"; *c; c++)
    if (ctx_mask & ((1u << ctx_to_idx((unsigned char)*c)) | (1u << (ctx_to_idx((unsigned char)*c) + 8)))) rep_ctx[nrep++] = *c;
  rep_ctx[nrep] = 0;
  *nsite = 0;
  EPI_TRY(epi_batch_cx_report_dev(b, nullptr, rep_ctx, s, nsite));
  const bool whole = b->last_kind == KIND_CX;
  b->last_kind = KIND_NONE;
  if (!whole)
    return fail(EPI_ERR_STATE, "%s: the batch is set up for a sharded report (the sharded form is not built)", who);
  return EPI_OK;
}

int het_cx_fetch(epi_batch *b, int64_t nsite, hipStream_t s, DevBuf &cx) {
  const size_t N = (size_t)nsite;
  EPI_TRY(cx.ensure(N * 6 * 4));
  int32_t *cols[6];
  for (int i = 0; i < 6; i++) cols[i] = cx.as<int32_t>() + (size_t)i * N;
  b->last_kind = KIND_CX;                                  // (for the fetch of the table that has just been made)
  const int rc = epi_batch_cx_fetch_dev(b, cols, s);
  b->last_kind = KIND_NONE;
  return rc;
}

int het_strand_table(epi_batch *b, int64_t nsite, hipStream_t s) {
  const size_t N = (size_t)nsite;
  const int64_t nb_sites = ((int64_t)N + HET_WG - 1) / HET_WG;
  EPI_TRY(check_grid(nb_sites, HET_WG, "heterogeneity site kernels"));
  SiteReportState &t = b->sites;
  EPI_TRY(t.rank.ensure(N * 4));
  EPI_TRY(t.flag.ensure(N * 4));
  EPI_TRY(t.key.ensure(N * 8));
  EPI_TRY(t.sctx.ensure(N));
  EPI_TRY(t.scal.ensure(64));
  const int32_t *cx = t.cx.as<int32_t>();
  uint32_t *nplus = &t.scalars()->nplus;
  uint32_t *flag = t.flag.as<uint32_t>(), *rank = t.rank.as<uint32_t>();
  hipLaunchKernelGGL(k_het_strand_flag, dim3((unsigned)nb_sites), dim3(HET_WG), 0, s, cx + N, (uint32_t)N, flag);
  EPI_TRY(scan_exclusive_u32(flag, rank, (int64_t)N, nplus, b->scan_tmp, s));
  hipLaunchKernelGGL(k_het_sites, dim3((unsigned)nb_sites), dim3(HET_WG), 0, s, cx, cx + N, cx + 2 * N, cx + 3 * N, rank, nplus,
                     (uint32_t)N, t.key.as<unsigned long long>(), t.sctx.as<uint8_t>());
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

int het_site_table(epi_batch *b, int64_t nsite, hipStream_t s) {
  EPI_TRY(check_grid((nsite + HET_WG - 1) / HET_WG, HET_WG, "heterogeneity site kernels"));
  EPI_TRY(het_cx_fetch(b, nsite, s, b->sites.cx));
  return het_strand_table(b, nsite, s);
}

int64_t het_counter_bytes(int64_t nsites, int k) {
  if (nsites < 0 || k < kHetMinK || k > kHetMaxK || nsites >= (1LL << 31)) return -1;
  const int64_t bytes = (nsites << k) * 4;
  return bytes > kHetCountsCap ? -1 : bytes;
}

int het_count_launch(const HetRows &rows, int k, uint32_t *counts, int64_t nb_rows, bool wide, hipStream_t s) {
  HetArgs a;
  static_cast<HetRows &>(a) = rows;
  a.k = k;
  a.counts = counts;
  if (wide) hipLaunchKernelGGL((k_het_count<64>), dim3((unsigned)nb_rows), dim3(HET_WG), 0, s, a);
  else hipLaunchKernelGGL((k_het_count<16>), dim3((unsigned)nb_rows), dim3(HET_WG), 0, s, a);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

void het_rows_args(const epi_batch *b, uint32_t ctx_mask, double max_oo, HetRows &a) {
  a.xm = b->xm; a.off = b->off; a.len = b->len; a.rname = b->rname; a.strand = b->strand; a.start = b->start; a.n = b->n;
  a.key = b->sites.key.as<unsigned long long>(); a.sctx = b->sites.sctx.as<uint8_t>(); a.n1 = &b->sites.scalars()->nplus;
  a.N = (uint32_t)b->sites.nsite;
  a.oom_mask = ((1u << 2) | (1u << 5) | (1u << 6) | (1u << 7)) & ~ctx_mask;           // rcpp_mhl_report.cpp:176-177
  a.oou_mask = ((1u << 10) | (1u << 13) | (1u << 14) | (1u << 15)) & ~ctx_mask;
  a.max_oo = max_oo;
}

static int het_report(epi_batch *b, const char *ctx, int k, double max_oo, int32_t min_reads, int32_t max_span, hipStream_t s,
                      int64_t *nrow_out) {
  SiteReportState &t = b->sites;
  // (a) the site table
  int64_t nsite = 0;
  EPI_TRY(het_cx_sites(b, ctx, s, "epi_batch_heterogeneity_report_dev", &nsite));
  t.nsite = nsite; t.k = k;
  t.min_reads = (uint32_t)(min_reads > 1 ? min_reads : 1);
  t.max_span = max_span;
  if (nsite < k) { b->last_kind = KIND_HET; b->last_nrow = 0; t.nsite = 0; return EPI_OK; }
  if (het_counter_bytes(nsite, k) < 0)
    return fail(EPI_ERR_ARG, "epi_batch_heterogeneity_report_dev: %lld sites x %d patterns need %lld bytes of counters, above the cap of %lld",
                (long long)nsite, 1 << k, (long long)((nsite << k) * 4), (long long)kHetCountsCap);
  const size_t N = (size_t)nsite;
  const int64_t nb_sites = ((int64_t)N + HET_WG - 1) / HET_WG;
  bool wide = false;
  const int64_t nb_rows = het_count_blocks(b, &wide);
  EPI_TRY(check_grid(nb_rows, HET_WG, "heterogeneity counting kernel"));
  EPI_TRY(het_site_table(b, nsite, s));
  EPI_TRY(t.counts.ensure((N << k) * 4));
  uint32_t *flag = t.flag.as<uint32_t>();

  // (b) the histograms
  EPI_HIP(hipMemsetAsync(t.counts.p, 0, (N << k) * 4, s));
  HetRows a;
  het_rows_args(b, ctx_mask_of(ctx), max_oo, a);
  prof_begin("het_count", s);
  const int rc_count = het_count_launch(a, k, t.counts.as<uint32_t>(), nb_rows, wide, s);
  prof_end("het_count", s);
  EPI_TRY(rc_count);

  // (c) which windows are reported, and where
  HetFinish f;
  het_finish_args(b, f);
  hipLaunchKernelGGL(k_het_keep, dim3((unsigned)nb_sites), dim3(HET_WG), 0, s, f, flag);
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
  EPI_TRY(site_fetch_begin("epi_batch_heterogeneity_fetch_dev", b, KIND_HET, false, d_icols, 7, d_dcols, 4, stream, &s, &nrow));
  if (nrow == 0) return EPI_OK;
  HetFinish f;
  het_finish_args(b, f);
  HetOut o;
  o.rname = d_icols[0]; o.strand = d_icols[1]; o.pos = d_icols[2]; o.end = d_icols[3]; o.context = d_icols[4];
  o.nreads = d_icols[5]; o.npatterns = d_icols[6];
  o.beta = d_dcols[0]; o.epipoly = d_dcols[1]; o.entropy = d_dcols[2]; o.pdr = d_dcols[3];
  o.counts = d_counts;
  const unsigned nb = (unsigned)(((int64_t)f.N + HET_WG - 1) / HET_WG);
  prof_begin("het_emit", s);
  hipLaunchKernelGGL(k_het_emit, dim3(nb), dim3(HET_WG), 0, s, f, b->sites.flag.as<uint32_t>(), b->sites.out.as<uint32_t>(), o);
  prof_end("het_emit", s);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

}  // extern "C"
