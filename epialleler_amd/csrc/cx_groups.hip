// Two groups of cytosine reports against each other per site, with replicates, and the distribution tails the tests need
// (include/epihip.h, epi_cx_groups_dev and epi_dist_tail_dev, has the definitions).  No reference interface is replaced.
// Stateless like cx_compare.hip: the call reads the caller's columns, takes its scratch for the length of the call and
// touches no batch.  All on the call's stream:
//  Tails    k_dist_tail: a thread per value runs dist_math.hpp's tail_of -- the host's arithmetic in the host's order.
//  Keys     k_cxg_key, one launch per sample: a thread per row checks the row against its predecessor (cx_table.hpp's order,
//           the one k_cxc_sorted checks) and its fields against the key's ranges, and writes the row's 64-bit
//           key, its index in the concatenation of the tables (a's first) as the sort's value, and its two counts.
//  Sort     radix_sort.hip's sort, in a SortPairs workspace, over the key's seven bytes.  The sort is stable, so a run of equal keys -- a site
//           -- lists its samples in sample order; a table has a key once, so a run has at most 64 entries.
//  Sites    k_cxg_flag: the thread of a run's first entry walks the run, counts the samples that count in either group and
//           flags the site as reported; pooled coverage beyond int32 at a reported site raises the overflow flag.  util.hip's
//           scan over the flags; ONE read of {unsorted, bad row / overflow, sites, rows}.
//  Rows     only when order, ranges, coverage and capacity hold: k_cxg_emit, the thread of a reported run's first entry walks
//           the run twice (sums and mean; then squared deviations and X2, which need the mean and the pooled beta) and writes
//           the site's 21 columns.  The samples' betas are recomputed in the second walk instead of being kept: no array, no
//           scratch memory.  The test is a kernel argument, one branch per site.
// The sort always runs its seven passes: which of the key's upper bytes are empty is known on the device only, and a second
// read-back to learn it would cost the synchronisation the one read above avoids.
#include "cx_table.hpp"
#include "radix_sort.hpp"
#include "fisher_math.hpp"
#include "dist_math.hpp"

namespace epi {

constexpr int CXG_WG = 256;
constexpr int CXG_MAX_GROUP = 32;                             // samples a side
constexpr int CXG_MAX_RUN = 2 * CXG_MAX_GROUP;                // entries of a site: one per sample
constexpr CxRowLimit CXG_MAX_ROWS = {(1LL << 32) - 1, "2^32 - 1"};   // of all samples together: the sort's values are 32-bit
constexpr uint32_t CXG_KEY_BYTES = 0x7Fu;                     // the key's 56 bits
constexpr uint32_t CXG_BAD_ROW = 1u, CXG_BAD_POOLED = 2u;     // bits of CxgScalars::bad

struct CxgScalars {                                           // what the kernels and the host exchange (64 bytes allocated)
  uint32_t unsorted;       // 1 + the last table found out of order (0: none)
  uint32_t bad;            // CXG_BAD_ROW: a field outside the key's ranges or a negative count; CXG_BAD_POOLED: pooled coverage
  uint32_t nsite;          // sites at which a sample counts
  uint32_t nrow;           // reported sites
};

// ---- tails -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(CXG_WG) void k_dist_tail(int32_t kind, const double *__restrict__ x, const double *__restrict__ df, int64_t n,
                                                      double *__restrict__ p) {
  const int64_t i = (int64_t)blockIdx.x * CXG_WG + threadIdx.x;
  if (i >= n) return;
  p[i] = dist::tail_of(kind, x[i], df[i]);
}

// ---- keys --------------------------------------------------------------------------------------------------------------

struct CxgRows {                       // [total] each
  uint64_t *key;
  uint32_t *val;
  int32_t *meth, *unmeth;
};

// one sample's table; base: where its rows go in the concatenation, index: the sample
__global__ __launch_bounds__(CXG_WG) void k_cxg_key(CxTab t, uint32_t base, uint32_t index, CxgRows o, CxgScalars *__restrict__ sc) {
  const uint32_t i = blockIdx.x * (uint32_t)CXG_WG + threadIdx.x;
  if (i >= t.n) return;
  const int32_t rname = t.rname[i], pos = t.pos[i], strand = t.strand[i], ctx = t.context[i], m = t.meth[i], u = t.unmeth[i];
  if (i > 0 && !cx_above(t, i)) atomicMax(&sc->unsorted, index + 1u);
  if (rname < 0 || rname > EPI_CXG_MAX_RNAME || pos < 0 || strand < 1 || strand > 2 || ctx < 0 || ctx > 7 || m < 0 || u < 0)
    atomicOr(&sc->bad, CXG_BAD_ROW);
  const uint32_t g = base + i;
  o.key[g] = ((uint64_t)(uint32_t)rname & (uint64_t)EPI_CXG_MAX_RNAME) << 35 | ((uint64_t)(uint32_t)pos & 0x7FFFFFFFull) << 4 |
             (uint64_t)((uint32_t)(strand - 1) & 1u) << 3 | (uint64_t)((uint32_t)ctx & 7u);
  o.val[g] = g;
  o.meth[g] = m;
  o.unmeth[g] = u;
}

// ---- sites -------------------------------------------------------------------------------------------------------------

struct CxgSorted {                     // the sorted pairs, the rows' counts (by concatenation index) and the call's arguments
  const uint64_t *key;
  const uint32_t *val;
  const int32_t *meth, *unmeth;
  uint32_t n;                          // rows of all samples
  uint32_t first_b;                    // concatenation index of b's first row: a value below it is a row of a
  int32_t min_cov, min_a, min_b, test;
};

// entries of the run that starts at sorted entry j (at most CXG_MAX_RUN: more means a table had a key twice, which the
// order check has flagged)
__device__ __forceinline__ uint32_t cxg_run(const CxgSorted &t, uint32_t j) {
  const uint64_t k = t.key[j];
  uint32_t len = 1;
  while (len < (uint32_t)CXG_MAX_RUN && j + len < t.n && t.key[j + len] == k) len++;
  return len;
}

__global__ __launch_bounds__(CXG_WG) void k_cxg_flag(CxgSorted t, uint32_t *__restrict__ flag, CxgScalars *__restrict__ sc) {
  const uint32_t j = blockIdx.x * (uint32_t)CXG_WG + threadIdx.x;
  uint32_t site = 0;
  if (j < t.n) {
    uint32_t rep = 0;
    if (j == 0 || t.key[j - 1] != t.key[j]) {
      const uint32_t len = cxg_run(t, j);
      int32_t na = 0, nb = 0;
      int64_t cov_a = 0, cov_b = 0;
      for (uint32_t e = 0; e < len; e++) {
        const uint32_t v = t.val[j + e];
        if (v >= t.n) continue;
        const int64_t cov = (int64_t)t.meth[v] + (int64_t)t.unmeth[v];
        if (cov < (int64_t)t.min_cov) continue;
        if (v < t.first_b) { na++; cov_a += cov; } else { nb++; cov_b += cov; }
      }
      site = na + nb > 0 ? 1u : 0u;
      rep = na >= t.min_a && nb >= t.min_b ? 1u : 0u;
      if (rep && (cov_a > 0x7FFFFFFFLL || cov_b > 0x7FFFFFFFLL)) atomicOr(&sc->bad, CXG_BAD_POOLED);
    }
    flag[j] = rep;
  }
  const uint32_t wsum = wave_sum_u32(site);                  // (every lane of the wave is here)
  if ((threadIdx.x & 63) == 0 && wsum) atomicAdd(&sc->nsite, wsum);
}

// ---- rows --------------------------------------------------------------------------------------------------------------

struct CxgOut {
  int32_t *icol[10];                   // rname, strand, pos, context, meth_a, unmeth_a, meth_b, unmeth_b, nsamples_a, nsamples_b
  double *dcol[11];                    // beta_a, beta_b, delta_beta, mean_beta_a, mean_beta_b, var_a, var_b, stat, df, phi, p
  uint32_t nrow;
};

__device__ __forceinline__ double cxg_dev_term(double x, double e) { return x == 0.0 ? e : fisher::bd0(x, e); }

__global__ __launch_bounds__(CXG_WG) void k_cxg_emit(CxgSorted t, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ off, CxgOut o) {
  const uint32_t j = blockIdx.x * (uint32_t)CXG_WG + threadIdx.x;
  if (j >= t.n || !flag[j]) return;
  const uint32_t r = off[j];
  if (r >= o.nrow) return;
  const double nan = __builtin_nan("");
  const uint32_t len = cxg_run(t, j);
  // first walk: pooled counts and the sums of the samples' betas, in sample order
  int64_t Ma = 0, Ua = 0, Mb = 0, Ub = 0;
  int32_t cnt_a = 0, cnt_b = 0;
  double sum_a = 0.0, sum_b = 0.0;
  for (uint32_t e = 0; e < len; e++) {
    const uint32_t v = t.val[j + e];
    if (v >= t.n) continue;
    const int64_t m = t.meth[v], u = t.unmeth[v];
    if (m + u < (int64_t)t.min_cov) continue;
    const double beta = (double)m / (double)(m + u);
    if (v < t.first_b) { Ma += m; Ua += u; cnt_a++; sum_a += beta; } else { Mb += m; Ub += u; cnt_b++; sum_b += beta; }
  }
  const double Na = (double)(Ma + Ua), Nb = (double)(Mb + Ub);
  const double beta_a = (double)Ma / Na, beta_b = (double)Mb / Nb;
  const double mean_a = sum_a / (double)cnt_a, mean_b = sum_b / (double)cnt_b;
  // second walk: squared deviations from the group's mean, and the Pearson statistic around the group's pooled beta
  double ss_a = 0.0, ss_b = 0.0, X2 = 0.0;
  for (uint32_t e = 0; e < len; e++) {
    const uint32_t v = t.val[j + e];
    if (v >= t.n) continue;
    const int64_t m = t.meth[v], u = t.unmeth[v];
    if (m + u < (int64_t)t.min_cov) continue;
    const bool in_a = v < t.first_b;
    const double dm = (double)m, dn = (double)(m + u);
    const double dev = dm / dn - (in_a ? mean_a : mean_b);
    if (in_a) ss_a += dev * dev; else ss_b += dev * dev;
    const double ph = in_a ? beta_a : beta_b;
    const double ex = dn * ph, den = ex * (1.0 - ph), res = dm - ex;
    if (den != 0.0) X2 += res * res / den;
  }
  const double var_a = cnt_a >= 2 ? ss_a / (double)(cnt_a - 1) : nan, var_b = cnt_b >= 2 ? ss_b / (double)(cnt_b - 1) : nan;

  double stat = nan, df = nan, phi = nan, p = nan;
  if (t.test == EPI_CXG_FISHER) {
    p = fisher::fisher_two_sided(Ma, Ua, Mb, Ub);
  } else if (t.test == EPI_CXG_WELCH) {
    if (cnt_a >= 2 && cnt_b >= 2) {
      const double va = var_a / (double)cnt_a, vb = var_b / (double)cnt_b, s2 = va + vb;
      if (s2 != 0.0) {
        stat = (mean_b - mean_a) / sqrt(s2);
        df = s2 * s2 / (va * va / (double)(cnt_a - 1) + vb * vb / (double)(cnt_b - 1));
        p = dist::tail_of(EPI_DIST_T2, stat, df);
      }
    }
  } else {
    const double N = (double)(Ma + Ua + Mb + Ub);
    const double p0 = (double)(Ma + Mb) / N, q0 = (double)(Ua + Ub) / N;
    const double G = 2.0 * (((cxg_dev_term((double)Ma, Na * p0) + cxg_dev_term((double)Ua, Na * q0)) + cxg_dev_term((double)Mb, Nb * p0)) +
                            cxg_dev_term((double)Ub, Nb * q0));
    if (t.test == EPI_CXG_LRT) {
      stat = G; df = 1.0;
      p = dist::tail_of(EPI_DIST_CHISQ, G, 1.0);
    } else {
      const int32_t n = cnt_a + cnt_b;
      df = (double)(n - 2);
      if (n > 2) {
        const double over = X2 / df;
        phi = over > 1.0 ? over : 1.0;
        stat = G / phi;
        p = dist::tail_of(EPI_DIST_F1, stat, df);
      }
    }
  }

  const uint64_t k = t.key[j];
  o.icol[0][r] = (int32_t)(k >> 35); o.icol[1][r] = (int32_t)((k >> 3) & 1u) + 1; o.icol[2][r] = (int32_t)((k >> 4) & 0x7FFFFFFFull);
  o.icol[3][r] = (int32_t)(k & 7u);
  o.icol[4][r] = (int32_t)Ma; o.icol[5][r] = (int32_t)Ua; o.icol[6][r] = (int32_t)Mb; o.icol[7][r] = (int32_t)Ub;
  o.icol[8][r] = cnt_a; o.icol[9][r] = cnt_b;
  o.dcol[0][r] = beta_a; o.dcol[1][r] = beta_b; o.dcol[2][r] = beta_b - beta_a;
  o.dcol[3][r] = mean_a; o.dcol[4][r] = mean_b; o.dcol[5][r] = var_a; o.dcol[6][r] = var_b;
  o.dcol[7][r] = stat; o.dcol[8][r] = df; o.dcol[9][r] = phi; o.dcol[10][r] = p;
}

// ---- host --------------------------------------------------------------------------------------------------------------

// The call's scratch for n rows, and what epi_cx_groups_scratch_bytes states: the sort's workspace, the rows' two counts, the
// scalars and the scan's block sums (over the rows' flags; the tables' are fewer)
struct CxgLayout : ScratchArena {
  size_t sort, counts, scal, scan;
  explicit CxgLayout(int64_t n) { sort = reserve(SortPairs::bytes((size_t)n)); counts = reserve((size_t)n * 8); scal = reserve(64); scan = reserve(scan_tmp_bytes(n)); }
};

struct CxgCall {
  const CxTab *tabs;
  int32_t n_a, n_b, min_cov, min_a, min_b, test;
  int32_t *const *icols;
  double *const *dcols;
  int64_t cap, total;
};

static int cx_groups(epi_engine *e, const CxgCall &c, hipStream_t s, int64_t *nsite_out, int64_t *nrow_out) {
  const char *who = "epi_cx_groups_dev";
  const int64_t n = c.total, nblk = (n + CXG_WG - 1) / CXG_WG;
  EPI_TRY(check_grid(nblk, CXG_WG, "cytosine group comparison kernels"));
  CxgLayout w(n);                                             // (goes when the call returns)
  EPI_TRY(w.alloc());
  uint64_t *sort_mem; CxgRows rows; CxgScalars *sc; uint32_t *scan;
  EPI_TRY(w.at(w.sort, &sort_mem)); EPI_TRY(w.at(w.counts, &rows.meth)); EPI_TRY(w.at(w.scal, &sc)); EPI_TRY(w.at(w.scan, &scan));
  SortPairs sort(sort_mem, (size_t)n);
  DevBuf scan_tmp = DevBuf::view(scan, scan_tmp_bytes(n));
  rows.key = sort.keys_in(); rows.val = sort.vals_in(); rows.unmeth = rows.meth + n;
  EPI_HIP(hipMemsetAsync(sc, 0, 64, s));

  prof_begin("cxg_key", s);
  int64_t base = 0, first_b = 0;
  for (int k = 0; k < c.n_a + c.n_b; k++) {
    if (k == c.n_a) first_b = base;
    const int64_t nk = c.tabs[k].n;
    if (nk == 0) continue;
    hipLaunchKernelGGL(k_cxg_key, dim3((unsigned)((nk + CXG_WG - 1) / CXG_WG)), dim3(CXG_WG), 0, s, c.tabs[k], (uint32_t)base, (uint32_t)k, rows, sc);
    base += nk;
  }
  prof_end("cxg_key", s);
  EPI_HIP(hipGetLastError());

  prof_begin("cxg_sort", s);
  const int rc_sort = sort.sort(CXG_KEY_BYTES, scan_tmp, s);
  prof_end("cxg_sort", s);
  EPI_TRY(rc_sort);

  CxgSorted t;
  t.key = sort.keys(); t.val = sort.vals(); t.meth = rows.meth; t.unmeth = rows.unmeth;
  t.n = (uint32_t)n; t.first_b = (uint32_t)first_b;
  t.min_cov = c.min_cov > 1 ? c.min_cov : 1; t.min_a = c.min_a; t.min_b = c.min_b; t.test = c.test;
  uint32_t *flag = sort.spare<uint32_t>(), *off = flag + n;
  prof_begin("cxg_flag", s);
  hipLaunchKernelGGL(k_cxg_flag, dim3((unsigned)nblk), dim3(CXG_WG), 0, s, t, flag, sc);
  const int rc_scan = scan_exclusive_u32(flag, off, n, &sc->nrow, scan_tmp, s);
  prof_end("cxg_flag", s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(rc_scan);

  CxgScalars h;                                               // the one synchronisation before anything is written
  EPI_TRY(read_scalars(e, s, sc, sizeof(h), &h));
  if (h.unsorted)
    return fail(EPI_ERR_ARG, "%s: the rows of table %u (counting a's, then b's, from 0) are not strictly ascending in (rname, pos, strand)", who, h.unsorted - 1u);
  if (h.bad & CXG_BAD_ROW)
    return fail(EPI_ERR_ARG, "%s: a row has an rname code outside 0 .. %d, a negative pos, a strand other than 1 and 2, a context code outside 0 .. 7 or a negative count",
                who, EPI_CXG_MAX_RNAME);
  *nsite_out = h.nsite;
  *nrow_out = h.nrow;
  if (h.bad & CXG_BAD_POOLED)
    return fail(EPI_ERR_ARG, "%s: a group's pooled meth + unmeth at a reported site exceeds 2^31 - 1, which an int32 column cannot hold", who);
  EPI_TRY(cx_rows_fit(who, "rows", h.nrow, c.cap));
  if (h.nrow == 0) return EPI_OK;
  EPI_TRY(cx_cols_arg(who, c.icols, 10, c.dcols, 11));
  CxgOut o;
  for (int i = 0; i < 10; i++) o.icol[i] = c.icols[i];
  for (int i = 0; i < 11; i++) o.dcol[i] = c.dcols[i];
  o.nrow = h.nrow;
  prof_begin("cxg_emit", s);
  hipLaunchKernelGGL(k_cxg_emit, dim3((unsigned)nblk), dim3(CXG_WG), 0, s, t, flag, off, o);
  prof_end("cxg_emit", s);
  EPI_HIP(hipGetLastError());
  EPI_HIP(hipStreamSynchronize(s));                           // (the scratch goes back when this returns)
  return EPI_OK;
}

}  // namespace epi

using namespace epi;

extern "C" {

int epi_dist_tail_dev(epi_engine *e, int32_t kind, const double *d_x, const double *d_df, int64_t n, double *d_p, void *stream) {
  const char *who = "epi_dist_tail_dev";
  if (!e) return fail(EPI_ERR_ARG, "%s: NULL engine", who);
  if (kind < EPI_DIST_CHISQ || kind > EPI_DIST_F1) return fail(EPI_ERR_ARG, "%s: kind = %d, one of EPI_DIST_CHISQ, EPI_DIST_T2, EPI_DIST_F1", who, kind);
  if (n < 0 || (n > 0 && (!d_x || !d_df || !d_p))) return fail(EPI_ERR_ARG, "%s: bad arguments", who);
  if (n == 0) return EPI_OK;
  const int64_t nb = (n + CXG_WG - 1) / CXG_WG;
  EPI_TRY(check_grid(nb, CXG_WG, "distribution tail kernel"));
  EPI_HIP(hipSetDevice(e->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  prof_begin("dist_tail", s);
  hipLaunchKernelGGL(k_dist_tail, dim3((unsigned)nb), dim3(CXG_WG), 0, s, kind, d_x, d_df, n, d_p);
  prof_end("dist_tail", s);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

int epi_cx_groups_scratch_bytes(int64_t total_rows, int64_t *bytes_out) {
  if (!bytes_out) return fail(EPI_ERR_ARG, "epi_cx_groups_scratch_bytes: NULL argument");
  *bytes_out = 0;
  EPI_TRY(cx_rows_arg("epi_cx_groups_scratch_bytes", total_rows, CXG_MAX_ROWS));
  if (total_rows > 0) *bytes_out = (int64_t)CxgLayout(total_rows).used;
  return EPI_OK;
}

int epi_cx_groups_dev(epi_engine *e, const int32_t *const *d_tabs, const int64_t *nrows, int32_t n_a, int32_t n_b, int32_t min_coverage,
                      int32_t min_samples_a, int32_t min_samples_b, int32_t test, int32_t *const d_icols[10], double *const d_dcols[11],
                      int64_t cap, void *stream, int64_t *nsite_out, int64_t *nrow_out) {
  const char *who = "epi_cx_groups_dev";
  if (!e || !nsite_out || !nrow_out) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  *nsite_out = 0; *nrow_out = 0;
  if (n_a < 1 || n_a > CXG_MAX_GROUP || n_b < 1 || n_b > CXG_MAX_GROUP)
    return fail(EPI_ERR_ARG, "%s: %d and %d samples, a group holds 1 to %d", who, n_a, n_b, CXG_MAX_GROUP);
  if (min_samples_a < 1 || min_samples_a > n_a || min_samples_b < 1 || min_samples_b > n_b)
    return fail(EPI_ERR_ARG, "%s: min_samples_a = %d and min_samples_b = %d, each from 1 to its group's size (%d, %d)", who, min_samples_a,
                min_samples_b, n_a, n_b);
  if (test < EPI_CXG_FISHER || test > EPI_CXG_WELCH) return fail(EPI_ERR_ARG, "%s: test = %d, one of EPI_CXG_FISHER, LRT, LRT_MN, WELCH", who, test);
  if (!d_tabs || !nrows) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  if (cap < 0) return fail(EPI_ERR_ARG, "%s: negative capacity", who);
  int64_t total = 0;
  CxTab tabs[CXG_MAX_RUN];
  for (int k = 0; k < n_a + n_b; k++) {
    char table[64];
    snprintf(table, sizeof table, "%s: table %d", who, k);
    EPI_TRY(cx_tab_arg(table, d_tabs + 6 * k, nrows[k], CXG_MAX_ROWS, &tabs[k]));
    total += nrows[k];
  }
  if (total > CXG_MAX_ROWS.rows) return fail(EPI_ERR_ARG, "%s: %lld rows in all, the samples hold fewer than 2^32 together", who, (long long)total);
  if (total == 0) return EPI_OK;
  EPI_HIP(hipSetDevice(e->device));
  CxgCall c;
  c.tabs = tabs; c.n_a = n_a; c.n_b = n_b; c.min_cov = min_coverage; c.min_a = min_samples_a; c.min_b = min_samples_b;
  c.test = test; c.icols = d_icols; c.dcols = d_dcols; c.cap = cap; c.total = total;
  return cx_groups(e, c, reinterpret_cast<hipStream_t>(stream), nsite_out, nrow_out);
}

}  // extern "C"
