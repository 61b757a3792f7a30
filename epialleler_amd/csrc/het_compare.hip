// Heterogeneity comparison: the epiallele histograms of two batches a and b over the windows of the sites they have in
// common, and what separates the two histograms of a window (include/epihip.h, epi_batch_heterogeneity_compare_dev, has the
// definitions).  No reference interface is replaced.  The counting is the heterogeneity report's (heterogeneity.hip; the
// shared parts are in site_table.hpp and het_common.hpp), twice, on one site table.  All on the call's stream:
//  (a) b's site table as a heterogeneity report makes it (its CX report, fetched into b's sites.cx, split per strand into
//      b's sites.key / sites.sctx); a's CX report, fetched into a's sites.cx_all.
//  (b) k_hetcmp_match: a thread per CX row of a searches the part of b's table for its strand (binary, keys of one
//      strand are sorted) and flags the row when b has the key with the same context code.  util.hip's scan, then
//      k_hetcmp_compact writes the flagged rows' rname, strand, pos and context into a's sites.cx: the common table, in
//      a's CX order.  site_strand_table turns it into the common per-strand table in a's sites.key / sites.sctx.
//  (c) k_het_count<16> / <64>, unchanged, once over a's rows into a's sites.counts and once over b's rows into a's
//      sites.counts_b, both with the common table.  The lane shape follows the batch whose rows are counted.
//  (d) k_hetcmp_keep (a thread per common site = per window start): n_a, n_b, min_reads, the span cap -> a flag; the scan;
//      k_hetcmp_emit (at fetch) writes het_metrics of either histogram, as k_het_emit does, and the comparison
//      metrics, every sum over the bins in ascending order inside one thread: no launch shape enters a result.
// Everything the fetch needs is in a's sites; b keeps its own site table and is left as site_cx_report leaves it (KIND_NONE).
#include "het_common.hpp"

namespace epi {

struct CmpMatch {
  const int32_t *rname, *strand, *pos, *context;   // a's CX table
  uint32_t Na;
  const unsigned long long *key_b;                 // b's per-strand table
  const uint8_t *sctx_b;
  const uint32_t *n1_b;
  uint32_t Nb;
};

__global__ __launch_bounds__(SITE_WG) void k_hetcmp_match(CmpMatch m, uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (i >= m.Na) return;
  const uint32_t n1 = *m.n1_b;
  const bool plus = m.strand[i] == 1;
  uint32_t lo = plus ? 0u : n1, hi = plus ? n1 : m.Nb;      // an empty part: nothing is searched, nothing is common
  const uint32_t end = hi;
  const unsigned long long key = table_key(m.rname[i], (int64_t)m.pos[i]);
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (m.key_b[mid] < key) lo = mid + 1u; else hi = mid;
  }
  flag[i] = lo < end && m.key_b[lo] == key && m.sctx_b[lo] == (uint8_t)m.context[i] ? 1u : 0u;
}

// row i of a's table (columns of Na rows) to row off[i] of the common one (columns of Nc rows)
__global__ __launch_bounds__(SITE_WG) void k_hetcmp_compact(const int32_t *__restrict__ src, uint32_t Na, const uint32_t *__restrict__ flag,
                                                          const uint32_t *__restrict__ off, int32_t *__restrict__ dst, uint32_t Nc) {
  const uint32_t i = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (i >= Na || !flag[i]) return;
  const uint32_t r = off[i];
  if (r >= Nc) return;
#pragma unroll
  for (int c = 0; c < 4; c++) dst[(size_t)c * Nc + r] = src[(size_t)c * Na + i];
}

struct CmpFinish : HetFinish {          // counts: a's side
  const uint32_t *counts_b;
};

__global__ __launch_bounds__(SITE_WG) void k_hetcmp_keep(CmpFinish f, uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (i >= f.N) return;
  int32_t end = 0;
  const uint32_t *ca = het_window(f, i, &end);
  uint32_t keep = 0;
  if (ca) {
    const uint32_t *cb = f.counts_b + (ca - f.counts);
    uint64_t na = 0, nb = 0;
    for (int b = 0; b < (1 << f.k); b++) { na += ca[b]; nb += cb[b]; }
    const int64_t span = (int64_t)end - (int64_t)f.pos[i] + 1;
    keep = na >= (uint64_t)f.min_reads && nb >= (uint64_t)f.min_reads && (f.max_span == 0 || span <= f.max_span) ? 1u : 0u;
  }
  flag[i] = keep;
}

struct CmpOut {
  int32_t *rname, *strand, *pos, *end, *context, *nreads[2], *npatterns[2], *df;
  double *beta[2], *entropy[2], *epipoly[2], *pdr[2];
  double *delta_beta, *delta_entropy, *jsd, *tvd, *g;
  int32_t *counts[2];                   // [nrow][2^k] or null
};

__global__ __launch_bounds__(SITE_WG) void k_hetcmp_emit(CmpFinish f, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ out_off,
                                                        CmpOut o) {
  const uint32_t i = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (i >= f.N || !flag[i]) return;
  int32_t end = 0;
  const uint32_t *ca = het_window(f, i, &end);
  if (!ca) return;
  const uint32_t *cb = f.counts_b + (ca - f.counts);
  const int nb = 1 << f.k;
  const uint32_t r = out_off[i];
  o.rname[r] = f.rname[i]; o.strand[r] = f.strand[i]; o.pos[r] = f.pos[i]; o.end[r] = end; o.context[r] = f.context[i];
  const uint32_t *const c[2] = {ca, cb};
  HetMetrics m[2];
#pragma unroll
  for (int side = 0; side < 2; side++) {                      // either sample's columns, as k_het_emit writes them
    m[side] = het_metrics(c[side], f.k, o.counts[side] ? o.counts[side] + ((size_t)r << f.k) : nullptr);
    o.nreads[side][r] = (int32_t)m[side].n; o.npatterns[side][r] = m[side].npatterns;
    o.beta[side][r] = m[side].beta; o.epipoly[side][r] = m[side].epipoly; o.entropy[side][r] = m[side].entropy; o.pdr[side][r] = m[side].pdr;
  }
  const double dna = (double)m[0].n, dnb = (double)m[1].n;
  o.delta_beta[r] = m[1].beta - m[0].beta;
  o.delta_entropy[r] = m[1].entropy - m[0].entropy;

  // the two histograms against each other: Jensen-Shannon divergence (bits), total variation distance, bins ascending
  int32_t nz = 0;
  double jsd = 0.0, tv = 0.0;
  for (int b = 0; b < nb; b++) {
    const uint32_t va = ca[b], vb = cb[b];
    nz += (va | vb) ? 1 : 0;
    const double p = (double)va / dna, q = (double)vb / dnb;
    const double m = (p + q) / 2.0;
    if (va) jsd += 0.5 * p * log2(p / m);
    if (vb) jsd += 0.5 * q * log2(q / m);
    tv += fabs(p - q);
  }
  jsd = jsd < 0.0 ? 0.0 : jsd > 1.0 ? 1.0 : jsd;
  // the likelihood-ratio statistic of the 2 x 2^k table: a's bins, then b's
  const double dtot = dna + dnb;
  double g = 0.0;
  for (int b = 0; b < nb; b++) {
    const uint32_t va = ca[b];
    if (va) g += (double)va * log((double)va / ((dna * (double)((uint64_t)va + cb[b])) / dtot));
  }
  for (int b = 0; b < nb; b++) {
    const uint32_t vb = cb[b];
    if (vb) g += (double)vb * log((double)vb / ((dnb * (double)((uint64_t)ca[b] + vb)) / dtot));
  }
  o.df[r] = nz - 1;
  o.jsd[r] = jsd;
  o.tvd[r] = 0.5 * tv;
  o.g[r] = 2.0 * g;
}

static void cmp_finish_args(const epi_batch *a, CmpFinish &f) {
  het_finish_args(a, f);
  f.counts_b = a->sites.cmp.counts_b.as<uint32_t>();
}

static int cmp_empty(epi_batch *a, int64_t ncommon, int64_t *ncommon_out) {
  a->last_kind = KIND_HETCMP; a->last_nrow = 0; a->sites.nsite = 0;
  *ncommon_out = ncommon;
  return EPI_OK;
}

static int het_compare(epi_batch *a, epi_batch *b, const char *ctx, int k, double max_oo, int32_t min_reads, int32_t max_span,
                       hipStream_t s, int64_t *ncommon_out, int64_t *nrow_out) {
  const char *who = "epi_batch_heterogeneity_compare_dev";
  SiteReportState &t = a->sites;
  // (a) the two site tables: b's as a report of its own has it, a's in CX row order only
  int64_t nsite_b = 0, nsite_a = 0;
  EPI_TRY(site_cx_report(b, ctx, s, who, &nsite_b));
  b->sites.nsite = 0;                                      // (b's buffers hold no report's table from here on)
  if (nsite_b > 0) {
    if (nsite_b >= (1LL << 31)) return fail(EPI_ERR_ARG, "%s: %lld sites in the second batch", who, (long long)nsite_b);
    EPI_TRY(site_table(b, nsite_b, s));
  }
  EPI_TRY(site_cx_report(a, ctx, s, who, &nsite_a));
  t.nsite = 0; t.het.k = k;
  t.min_reads = (uint32_t)(min_reads > 1 ? min_reads : 1);
  t.het.max_span = max_span;
  if (nsite_a == 0 || nsite_b == 0) return cmp_empty(a, 0, ncommon_out);
  if (nsite_a >= (1LL << 31)) return fail(EPI_ERR_ARG, "%s: %lld sites in the first batch", who, (long long)nsite_a);
  const size_t Na = (size_t)nsite_a;
  const int64_t nb_a = ((int64_t)Na + SITE_WG - 1) / SITE_WG;
  EPI_TRY(check_grid(nb_a, SITE_WG, "heterogeneity comparison site kernels"));
  EPI_TRY(site_cx_fetch(a, nsite_a, s, t.cmp.cx_all));
  EPI_TRY(t.flag.ensure(Na * 4));
  EPI_TRY(t.out.ensure(Na * 4));
  EPI_TRY(t.scal.ensure(64));
  uint32_t *flag = t.flag.as<uint32_t>(), *out = t.out.as<uint32_t>();

  // (b) the sites of a that b has too
  const int32_t *cx_a = t.cmp.cx_all.as<int32_t>();
  CmpMatch m;
  m.rname = cx_a; m.strand = cx_a + Na; m.pos = cx_a + 2 * Na; m.context = cx_a + 3 * Na;
  m.Na = (uint32_t)Na;
  m.key_b = b->sites.key.as<unsigned long long>(); m.sctx_b = b->sites.sctx.as<uint8_t>(); m.n1_b = &b->sites.scalars()->nplus;
  m.Nb = (uint32_t)nsite_b;
  prof_begin("hetcmp_intersect", s);
  hipLaunchKernelGGL(k_hetcmp_match, dim3((unsigned)nb_a), dim3(SITE_WG), 0, s, m, flag);
  int64_t ncommon = 0;
  EPI_TRY(site_rows(a, flag, (int64_t)Na, out, &t.scalars()->ncommon, s, &ncommon, "hetcmp_intersect"));
  if (ncommon < k) return cmp_empty(a, ncommon, ncommon_out);
  const int64_t cbytes = het_counter_bytes(ncommon, k);
  if (cbytes < 0)
    return fail(EPI_ERR_ARG, "%s: %lld common sites x %d patterns need %lld bytes of counters per batch, above the cap", who,
                (long long)ncommon, 1 << k, (long long)((ncommon << k) * 4));
  const size_t Nc = (size_t)ncommon;
  EPI_TRY(t.cx.ensure(Nc * 6 * 4));
  prof_begin("hetcmp_compact", s);
  hipLaunchKernelGGL(k_hetcmp_compact, dim3((unsigned)nb_a), dim3(SITE_WG), 0, s, cx_a, (uint32_t)Na, flag, out, t.cx.as<int32_t>(),
                     (uint32_t)Nc);
  const int rc_table = site_strand_table(a, ncommon, s);
  prof_end("hetcmp_compact", s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(rc_table);
  t.nsite = ncommon;
  *ncommon_out = ncommon;

  // (c) both batches' histograms over the common table
  bool wide_a = false, wide_b = false;
  const int64_t nb_rows_a = site_count_blocks(a, &wide_a), nb_rows_b = site_count_blocks(b, &wide_b);
  EPI_TRY(check_grid(nb_rows_a, SITE_WG, "heterogeneity counting kernel"));
  EPI_TRY(check_grid(nb_rows_b, SITE_WG, "heterogeneity counting kernel"));
  EPI_TRY(t.counts.ensure((size_t)cbytes));
  EPI_TRY(t.cmp.counts_b.ensure((size_t)cbytes));
  EPI_HIP(hipMemsetAsync(t.counts.p, 0, (size_t)cbytes, s));
  EPI_HIP(hipMemsetAsync(t.cmp.counts_b.p, 0, (size_t)cbytes, s));
  const uint32_t ctx_mask = ctx_mask_of(ctx);
  SiteRows ra, rb;
  site_rows_args(a, ctx_mask, max_oo, ra);
  site_rows_args(b, ctx_mask, max_oo, rb);
  rb.key = ra.key; rb.sctx = ra.sctx; rb.n1 = ra.n1; rb.N = ra.N;     // b's rows, the common table
  prof_begin("hetcmp_count_a", s);
  const int rc_a = het_count_launch(ra, k, t.counts.as<uint32_t>(), nb_rows_a, wide_a, s);
  prof_end("hetcmp_count_a", s);
  EPI_TRY(rc_a);
  prof_begin("hetcmp_count_b", s);
  const int rc_b = het_count_launch(rb, k, t.cmp.counts_b.as<uint32_t>(), nb_rows_b, wide_b, s);
  prof_end("hetcmp_count_b", s);
  EPI_TRY(rc_b);

  // (d) which windows are reported, and where
  const int64_t nb_c = ((int64_t)Nc + SITE_WG - 1) / SITE_WG;
  CmpFinish f;
  cmp_finish_args(a, f);
  flag = t.flag.as<uint32_t>();                              // (site_strand_table is done with its Nc words)
  prof_begin("hetcmp_keep", s);
  hipLaunchKernelGGL(k_hetcmp_keep, dim3((unsigned)nb_c), dim3(SITE_WG), 0, s, f, flag);
  EPI_TRY(site_rows(a, flag, (int64_t)Nc, t.out.as<uint32_t>(), &t.scalars()->nrow, s, nrow_out, "hetcmp_keep"));
  a->last_kind = KIND_HETCMP;
  a->last_nrow = *nrow_out;
  return EPI_OK;
}

}  // namespace epi

using namespace epi;

extern "C" {

int epi_batch_heterogeneity_compare_dev(epi_batch *a, epi_batch *b, const char *ctx, int k, double max_ooctx_meth_frac,
                                        int32_t min_reads, int32_t max_window_span, void *stream, int64_t *ncommon_out,
                                        int64_t *nrow_out) {
  if (!a || !b || !ctx || !ncommon_out || !nrow_out) return fail(EPI_ERR_ARG, "epi_batch_heterogeneity_compare_dev: NULL argument");
  *ncommon_out = 0; *nrow_out = 0;
  if (a->eng != b->eng) return fail(EPI_ERR_ARG, "epi_batch_heterogeneity_compare_dev: the two batches are of different engines");
  EPI_TRY(het_check_window("epi_batch_heterogeneity_compare_dev", k, max_window_span));
  a->last_kind = KIND_NONE;
  b->last_kind = KIND_NONE;
  EPI_HIP(hipSetDevice(a->eng->device));
  return het_compare(a, b, ctx, k, max_ooctx_meth_frac, min_reads, max_window_span, pick_stream(a, stream), ncommon_out, nrow_out);
}

int epi_batch_heterogeneity_compare_fetch_dev(epi_batch *a, int32_t *const d_icols[10], double *const d_dcols[13],
                                              int32_t *d_counts_a, int32_t *d_counts_b, void *stream) {
  hipStream_t s = nullptr;
  int64_t nrow = 0;
  EPI_TRY(site_fetch_begin("epi_batch_heterogeneity_compare_fetch_dev", a, KIND_HETCMP, "heterogeneity comparison", false, d_icols, 10, d_dcols, 13, stream, &s,
                           &nrow));
  if (nrow == 0) return EPI_OK;
  CmpFinish f;
  cmp_finish_args(a, f);
  CmpOut o;
  o.rname = d_icols[0]; o.strand = d_icols[1]; o.pos = d_icols[2]; o.end = d_icols[3]; o.context = d_icols[4];
  o.nreads[0] = d_icols[5]; o.nreads[1] = d_icols[6]; o.npatterns[0] = d_icols[7]; o.npatterns[1] = d_icols[8]; o.df = d_icols[9];
  for (int side = 0; side < 2; side++) {
    o.beta[side] = d_dcols[side]; o.entropy[side] = d_dcols[2 + side]; o.epipoly[side] = d_dcols[4 + side]; o.pdr[side] = d_dcols[6 + side];
  }
  o.delta_beta = d_dcols[8]; o.delta_entropy = d_dcols[9]; o.jsd = d_dcols[10]; o.tvd = d_dcols[11]; o.g = d_dcols[12];
  o.counts[0] = d_counts_a; o.counts[1] = d_counts_b;
  const unsigned nb = (unsigned)(((int64_t)f.N + SITE_WG - 1) / SITE_WG);
  prof_begin("hetcmp_emit", s);
  hipLaunchKernelGGL(k_hetcmp_emit, dim3(nb), dim3(SITE_WG), 0, s, f, a->sites.flag.as<uint32_t>(), a->sites.out.as<uint32_t>(), o);
  prof_end("hetcmp_emit", s);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

}  // extern "C"
