// Heterogeneity comparison: the epiallele histograms of two batches a and b over the windows of the sites they have in
// common, and what separates the two histograms of a window (include/epihip.h, epi_batch_heterogeneity_compare_dev, has the
// definitions).  No reference interface is replaced.  The counting is the heterogeneity report's (heterogeneity.hip; the
// shared parts are in het_common.hpp), twice, on one site table.  All on the call's stream:
//  (a) b's site table as a heterogeneity report makes it (its CX report, fetched into b's het_cx, split per strand into
//      b's het_key / het_sctx); a's CX report, fetched into a's cmp_cx.
//  (b) k_hetcmp_match: a thread per CX row of a searches the part of b's table for its strand (binary, keys of one
//      strand are sorted) and flags the row when b has the key with the same context code.  util.hip's scan, then
//      k_hetcmp_compact writes the flagged rows' rname, strand, pos and context into a's het_cx: the common table, in
//      a's CX order.  het_strand_table turns it into the common per-strand table in a's het_key / het_sctx.
//  (c) k_het_count<16> / <64>, unchanged, once over a's rows into a's het_counts and once over b's rows into a's
//      cmp_counts_b, both with the common table.  The lane shape follows the batch whose rows are counted.
//  (d) k_hetcmp_keep (a thread per common site = per window start): n_a, n_b, min_reads, the span cap -> a flag; the scan;
//      k_hetcmp_emit (at fetch) computes the per-sample metrics in k_het_emit's order of operations and the comparison
//      metrics, every sum over the bins in ascending order inside one thread: no launch shape enters a result.
// Everything the fetch needs is a's; b keeps its own site table and is left as het_cx_sites leaves it (KIND_NONE).
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

__global__ __launch_bounds__(HET_WG) void k_hetcmp_match(CmpMatch m, uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * (uint32_t)HET_WG + threadIdx.x;
  if (i >= m.Na) return;
  const uint32_t n1 = *m.n1_b;
  const bool plus = m.strand[i] == 1;
  uint32_t lo = plus ? 0u : n1, hi = plus ? n1 : m.Nb;      // an empty part: nothing is searched, nothing is common
  const uint32_t end = hi;
  const unsigned long long key = het_key(m.rname[i], (int64_t)m.pos[i]);
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (m.key_b[mid] < key) lo = mid + 1u; else hi = mid;
  }
  flag[i] = lo < end && m.key_b[lo] == key && m.sctx_b[lo] == (uint8_t)m.context[i] ? 1u : 0u;
}

// row i of a's table (columns of Na rows) to row off[i] of the common one (columns of Nc rows)
__global__ __launch_bounds__(HET_WG) void k_hetcmp_compact(const int32_t *__restrict__ src, uint32_t Na, const uint32_t *__restrict__ flag,
                                                          const uint32_t *__restrict__ off, int32_t *__restrict__ dst, uint32_t Nc) {
  const uint32_t i = blockIdx.x * (uint32_t)HET_WG + threadIdx.x;
  if (i >= Na || !flag[i]) return;
  const uint32_t r = off[i];
  if (r >= Nc) return;
#pragma unroll
  for (int c = 0; c < 4; c++) dst[(size_t)c * Nc + r] = src[(size_t)c * Na + i];
}

struct CmpFinish : HetFinish {          // counts: a's side
  const uint32_t *counts_b;
};

__global__ __launch_bounds__(HET_WG) void k_hetcmp_keep(CmpFinish f, uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * (uint32_t)HET_WG + threadIdx.x;
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

// one sample's columns of output row r, as k_het_emit computes them; returns n
__device__ __forceinline__ uint64_t hetcmp_sample(const uint32_t *c, int k, uint32_t r, const CmpOut &o, int side, double *beta_out,
                                                  double *entropy_out) {
  const int nb = 1 << k;
  uint64_t n = 0, nmeth = 0;
  int32_t npat = 0;
  for (int b = 0; b < nb; b++) { const uint32_t v = c[b]; n += v; nmeth += (uint64_t)v * (uint32_t)__popc(b); npat += v ? 1 : 0; }
  const double dn = (double)n;
  double sq = 0.0, ent = 0.0;
  int32_t *oc = o.counts[side];
  for (int b = 0; b < nb; b++) {                              // ascending bins
    const uint32_t v = c[b];
    if (oc) oc[(size_t)r * nb + b] = (int32_t)v;
    if (!v) continue;
    const double pb = (double)v / dn;
    sq += pb * pb;
    ent += pb * log2(pb);
  }
  o.nreads[side][r] = (int32_t)n; o.npatterns[side][r] = npat;
  *beta_out = (double)nmeth / (dn * (double)k);
  *entropy_out = -ent / (double)k;
  o.beta[side][r] = *beta_out;
  o.epipoly[side][r] = 1.0 - sq;
  o.entropy[side][r] = *entropy_out;
  o.pdr[side][r] = 1.0 - (double)((uint64_t)c[0] + c[nb - 1]) / dn;
  return n;
}

__global__ __launch_bounds__(HET_WG) void k_hetcmp_emit(CmpFinish f, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ out_off,
                                                        CmpOut o) {
  const uint32_t i = blockIdx.x * (uint32_t)HET_WG + threadIdx.x;
  if (i >= f.N || !flag[i]) return;
  int32_t end = 0;
  const uint32_t *ca = het_window(f, i, &end);
  if (!ca) return;
  const uint32_t *cb = f.counts_b + (ca - f.counts);
  const int nb = 1 << f.k;
  const uint32_t r = out_off[i];
  o.rname[r] = f.rname[i]; o.strand[r] = f.strand[i]; o.pos[r] = f.pos[i]; o.end[r] = end; o.context[r] = f.context[i];
  double beta_a, beta_b, ent_a, ent_b;
  const double dna = (double)hetcmp_sample(ca, f.k, r, o, 0, &beta_a, &ent_a);
  const double dnb = (double)hetcmp_sample(cb, f.k, r, o, 1, &beta_b, &ent_b);
  o.delta_beta[r] = beta_b - beta_a;
  o.delta_entropy[r] = ent_b - ent_a;

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
  f.counts_b = a->cmp_counts_b.as<uint32_t>();
}

static int cmp_empty(epi_batch *a, int64_t ncommon, int64_t *ncommon_out) {
  a->last_kind = KIND_HETCMP; a->last_nrow = 0; a->het_nsite = 0;
  *ncommon_out = ncommon;
  return EPI_OK;
}

static int het_compare(epi_batch *a, epi_batch *b, const char *ctx, int k, double max_oo, int32_t min_reads, int32_t max_span,
                       hipStream_t s, int64_t *ncommon_out, int64_t *nrow_out) {
  const char *who = "epi_batch_heterogeneity_compare_dev";
  // (a) the two site tables: b's as a report of its own has it, a's in CX row order only
  int64_t nsite_b = 0, nsite_a = 0;
  EPI_TRY(het_cx_sites(b, ctx, s, who, &nsite_b));
  b->het_nsite = 0;                                        // (b's buffers hold no report's table from here on)
  if (nsite_b > 0) {
    if (nsite_b >= (1LL << 31)) return fail(EPI_ERR_ARG, "%s: %lld sites in the second batch", who, (long long)nsite_b);
    EPI_TRY(het_site_table(b, nsite_b, s));
  }
  EPI_TRY(het_cx_sites(a, ctx, s, who, &nsite_a));
  a->het_nsite = 0; a->het_k = k;
  a->het_min_reads = (uint32_t)(min_reads > 1 ? min_reads : 1);
  a->het_max_span = max_span;
  if (nsite_a == 0 || nsite_b == 0) return cmp_empty(a, 0, ncommon_out);
  if (nsite_a >= (1LL << 31)) return fail(EPI_ERR_ARG, "%s: %lld sites in the first batch", who, (long long)nsite_a);
  const size_t Na = (size_t)nsite_a;
  const int64_t nb_a = ((int64_t)Na + HET_WG - 1) / HET_WG;
  EPI_TRY(check_grid(nb_a, HET_WG, "heterogeneity comparison site kernels"));
  EPI_TRY(het_cx_fetch(a, nsite_a, s, a->cmp_cx));
  EPI_TRY(a->het_flag.ensure(Na * 4));
  EPI_TRY(a->het_out.ensure(Na * 4));
  EPI_TRY(a->het_scal.ensure(64));
  uint32_t *scal = a->het_scal.as<uint32_t>();             // [0] '+' sites, [1] reported rows, [3] common sites
  uint32_t *flag = a->het_flag.as<uint32_t>(), *out = a->het_out.as<uint32_t>();

  // (b) the sites of a that b has too
  const int32_t *cx_a = a->cmp_cx.as<int32_t>();
  CmpMatch m;
  m.rname = cx_a; m.strand = cx_a + Na; m.pos = cx_a + 2 * Na; m.context = cx_a + 3 * Na;
  m.Na = (uint32_t)Na;
  m.key_b = b->het_key.as<unsigned long long>(); m.sctx_b = b->het_sctx.as<uint8_t>(); m.n1_b = b->het_scal.as<uint32_t>();
  m.Nb = (uint32_t)nsite_b;
  prof_begin("hetcmp_intersect", s);
  hipLaunchKernelGGL(k_hetcmp_match, dim3((unsigned)nb_a), dim3(HET_WG), 0, s, m, flag);
  const int rc_scan = scan_exclusive_u32(flag, out, (int64_t)Na, &scal[3], a->scan_tmp, s);
  prof_end("hetcmp_intersect", s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(rc_scan);
  uint32_t h_common = 0;
  EPI_TRY(read_scalars(a, s, &scal[3], sizeof(h_common), &h_common));
  const int64_t ncommon = h_common;
  if (ncommon < k) return cmp_empty(a, ncommon, ncommon_out);
  const int64_t cbytes = het_counter_bytes(ncommon, k);
  if (cbytes < 0)
    return fail(EPI_ERR_ARG, "%s: %lld common sites x %d patterns need %lld bytes of counters per batch, above the cap", who,
                (long long)ncommon, 1 << k, (long long)((ncommon << k) * 4));
  const size_t Nc = (size_t)ncommon;
  EPI_TRY(a->het_cx.ensure(Nc * 6 * 4));
  prof_begin("hetcmp_compact", s);
  hipLaunchKernelGGL(k_hetcmp_compact, dim3((unsigned)nb_a), dim3(HET_WG), 0, s, cx_a, (uint32_t)Na, flag, out, a->het_cx.as<int32_t>(),
                     (uint32_t)Nc);
  const int rc_table = het_strand_table(a, ncommon, s);
  prof_end("hetcmp_compact", s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(rc_table);
  a->het_nsite = ncommon;
  *ncommon_out = ncommon;

  // (c) both batches' histograms over the common table
  bool wide_a = false, wide_b = false;
  const int64_t nb_rows_a = het_count_blocks(a, &wide_a), nb_rows_b = het_count_blocks(b, &wide_b);
  EPI_TRY(check_grid(nb_rows_a, HET_WG, "heterogeneity counting kernel"));
  EPI_TRY(check_grid(nb_rows_b, HET_WG, "heterogeneity counting kernel"));
  EPI_TRY(a->het_counts.ensure((size_t)cbytes));
  EPI_TRY(a->cmp_counts_b.ensure((size_t)cbytes));
  EPI_HIP(hipMemsetAsync(a->het_counts.p, 0, (size_t)cbytes, s));
  EPI_HIP(hipMemsetAsync(a->cmp_counts_b.p, 0, (size_t)cbytes, s));
  const uint32_t ctx_mask = ctx_mask_of(ctx);
  HetRows ra, rb;
  het_rows_args(a, ctx_mask, max_oo, ra);
  het_rows_args(b, ctx_mask, max_oo, rb);
  rb.key = ra.key; rb.sctx = ra.sctx; rb.n1 = ra.n1; rb.N = ra.N;     // b's rows, the common table
  prof_begin("hetcmp_count_a", s);
  const int rc_a = het_count_launch(ra, k, a->het_counts.as<uint32_t>(), nb_rows_a, wide_a, s);
  prof_end("hetcmp_count_a", s);
  EPI_TRY(rc_a);
  prof_begin("hetcmp_count_b", s);
  const int rc_b = het_count_launch(rb, k, a->cmp_counts_b.as<uint32_t>(), nb_rows_b, wide_b, s);
  prof_end("hetcmp_count_b", s);
  EPI_TRY(rc_b);

  // (d) which windows are reported, and where
  const int64_t nb_c = ((int64_t)Nc + HET_WG - 1) / HET_WG;
  CmpFinish f;
  cmp_finish_args(a, f);
  flag = a->het_flag.as<uint32_t>();                         // (het_strand_table is done with its Nc words)
  prof_begin("hetcmp_keep", s);
  hipLaunchKernelGGL(k_hetcmp_keep, dim3((unsigned)nb_c), dim3(HET_WG), 0, s, f, flag);
  const int rc_keep = scan_exclusive_u32(flag, a->het_out.as<uint32_t>(), (int64_t)Nc, &scal[1], a->scan_tmp, s);
  prof_end("hetcmp_keep", s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(rc_keep);
  uint32_t h[2];
  EPI_TRY(read_scalars(a, s, scal, sizeof(h), h));
  a->last_kind = KIND_HETCMP;
  a->last_nrow = h[1];
  *nrow_out = h[1];
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
  if (k < kHetMinK || k > kHetMaxK)
    return fail(EPI_ERR_ARG, "epi_batch_heterogeneity_compare_dev: k = %d, windows hold %d to %d sites", k, kHetMinK, kHetMaxK);
  if (max_window_span < 0) return fail(EPI_ERR_ARG, "epi_batch_heterogeneity_compare_dev: negative max_window_span");
  a->last_kind = KIND_NONE;
  b->last_kind = KIND_NONE;
  EPI_HIP(hipSetDevice(a->eng->device));
  return het_compare(a, b, ctx, k, max_ooctx_meth_frac, min_reads, max_window_span, pick_stream(a, stream), ncommon_out, nrow_out);
}

int epi_batch_heterogeneity_compare_fetch_dev(epi_batch *a, int32_t *const d_icols[10], double *const d_dcols[13],
                                              int32_t *d_counts_a, int32_t *d_counts_b, void *stream) {
  if (!a || !d_icols || !d_dcols) return fail(EPI_ERR_ARG, "epi_batch_heterogeneity_compare_fetch_dev: NULL argument");
  if (a->last_kind != KIND_HETCMP)
    return fail(EPI_ERR_STATE, "epi_batch_heterogeneity_compare_fetch_dev: no finished heterogeneity comparison on this batch");
  if (a->last_nrow == 0) return EPI_OK;
  for (int i = 0; i < 10; i++) if (!d_icols[i]) return fail(EPI_ERR_ARG, "epi_batch_heterogeneity_compare_fetch_dev: NULL column");
  for (int i = 0; i < 13; i++) if (!d_dcols[i]) return fail(EPI_ERR_ARG, "epi_batch_heterogeneity_compare_fetch_dev: NULL column");
  EPI_HIP(hipSetDevice(a->eng->device));
  hipStream_t s = pick_stream(a, stream);
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
  const unsigned nb = (unsigned)(((int64_t)f.N + HET_WG - 1) / HET_WG);
  prof_begin("hetcmp_emit", s);
  hipLaunchKernelGGL(k_hetcmp_emit, dim3(nb), dim3(HET_WG), 0, s, f, a->het_flag.as<uint32_t>(), a->het_out.as<uint32_t>(), o);
  prof_end("hetcmp_emit", s);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

}  // extern "C"
