// Two cytosine reports against each other per site, and the regions in which they differ (include/epihip.h,
// epi_fisher_exact_dev, epi_cx_compare_dev, epi_cx_compare_regions_dev, has the definitions).  No reference interface is
// replaced.  The calls are stateless: they read the caller's columns, take their scratch for the length of the call and
// touch no batch.  All on the call's stream:
//  Fisher   k_fisher: a thread per table runs fisher_math.hpp's fisher_two_sided -- the host's arithmetic, in the host's
//           order, inside one thread: no LDS, no cross-lane work, no launch shape in a result.
//  Sites    k_cxc_sorted (both tables: every row above its predecessor, cx_table.hpp's order); k_cxc_match: a thread per
//           row of a searches b (binary, on the same key) and flags the row as common when b has the key with the same
//           context code, and as reported when both sides have the coverage; util.hip's scan over the reported flags; one
//           read of {unsorted a, unsorted b, common, reported}; then, and only when the order and the capacity hold,
//           k_cxc_emit writes the reported rows' integer columns and betas in a's order and k_fisher their p-values.
//  Regions  a run is a maximal stretch of significant rows of one direction and rname whose neighbours are at most max_gap
//           apart; k_reg_flag: a thread per row decides whether a run starts there and walks at most min_sites rows of it to
//           see whether it is reported; the scan; k_reg_emit: the thread of a reported run's first row walks the run once,
//           summing in ascending row order (a table that is one long run is walked by one thread).
#include "cx_table.hpp"
#include "fisher_math.hpp"

namespace epi {

constexpr int CXC_WG = 256;

// ---- Fisher ------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double fisher_cells(int64_t a, int64_t b, int64_t c, int64_t d) {
  if (a < 0 || b < 0 || c < 0 || d < 0) return __builtin_nan("");
  return fisher::fisher_two_sided(a, b, c, d);
}

__global__ __launch_bounds__(CXC_WG) void k_fisher(const int32_t *__restrict__ a, const int32_t *__restrict__ b,
                                                   const int32_t *__restrict__ c, const int32_t *__restrict__ d, int64_t n,
                                                   double *__restrict__ p) {
  const int64_t i = (int64_t)blockIdx.x * CXC_WG + threadIdx.x;
  if (i >= n) return;
  p[i] = fisher_cells(a[i], b[i], c[i], d[i]);
}

static int fisher_launch(const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d, int64_t n, double *p, hipStream_t s) {
  const int64_t nb = (n + CXC_WG - 1) / CXC_WG;
  EPI_TRY(check_grid(nb, CXC_WG, "Fisher kernel"));
  prof_begin("fisher_exact", s);
  hipLaunchKernelGGL(k_fisher, dim3((unsigned)nb), dim3(CXC_WG), 0, s, a, b, c, d, n, p);
  prof_end("fisher_exact", s);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

// ---- sites -------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(CXC_WG) void k_cxc_sorted(CxTab t, uint32_t *__restrict__ unsorted) {
  const uint32_t i = blockIdx.x * (uint32_t)CXC_WG + threadIdx.x;
  if (i == 0 || i >= t.n) return;
  if (!cx_above(t, i)) atomicOr(unsorted, 1u);
}

__device__ __forceinline__ bool cxc_covered(int32_t meth, int32_t unmeth, int32_t min_cov) {
  return (int64_t)meth + (int64_t)unmeth >= (int64_t)min_cov;
}

// keep[i]: row i of a is reported; brow[i]: the row of b it is matched to (meaningful where keep[i]); *ncommon: common rows
__global__ __launch_bounds__(CXC_WG) void k_cxc_match(CxTab a, CxTab b, int32_t min_cov, uint32_t *__restrict__ keep,
                                                      uint32_t *__restrict__ brow, uint32_t *__restrict__ ncommon) {
  const uint32_t i = blockIdx.x * (uint32_t)CXC_WG + threadIdx.x;
  uint32_t common = 0;
  if (i < a.n) {
    const int32_t rname = a.rname[i], pos = a.pos[i], strand = a.strand[i];
    uint32_t lo = 0, hi = b.n;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2u;
      if (cx_cmp(b, mid, rname, pos, strand) < 0) lo = mid + 1u; else hi = mid;
    }
    common = lo < b.n && cx_cmp(b, lo, rname, pos, strand) == 0 && b.context[lo] == a.context[i] ? 1u : 0u;
    const bool rep = common && cxc_covered(a.meth[i], a.unmeth[i], min_cov) && cxc_covered(b.meth[lo], b.unmeth[lo], min_cov);
    keep[i] = rep ? 1u : 0u;
    brow[i] = lo;
  }
  const uint32_t wsum = wave_sum_u32(common);              // (every lane of the wave is here)
  if ((threadIdx.x & 63) == 0 && wsum) atomicAdd(ncommon, wsum);
}

struct CxcOut {
  int32_t *rname, *strand, *pos, *context, *meth_a, *unmeth_a, *meth_b, *unmeth_b;
  double *beta_a, *beta_b, *delta_beta;
  uint32_t nrow;
};

__global__ __launch_bounds__(CXC_WG) void k_cxc_emit(CxTab a, CxTab b, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ off,
                                                     const uint32_t *__restrict__ brow, CxcOut o) {
  const uint32_t i = blockIdx.x * (uint32_t)CXC_WG + threadIdx.x;
  if (i >= a.n || !keep[i]) return;
  const uint32_t r = off[i], j = brow[i];
  if (r >= o.nrow || j >= b.n) return;
  const int32_t ma = a.meth[i], ua = a.unmeth[i], mb = b.meth[j], ub = b.unmeth[j];
  o.rname[r] = a.rname[i]; o.strand[r] = a.strand[i]; o.pos[r] = a.pos[i]; o.context[r] = a.context[i];
  o.meth_a[r] = ma; o.unmeth_a[r] = ua; o.meth_b[r] = mb; o.unmeth_b[r] = ub;
  const double beta_a = (double)ma / (double)((int64_t)ma + (int64_t)ua);
  const double beta_b = (double)mb / (double)((int64_t)mb + (int64_t)ub);
  o.beta_a[r] = beta_a; o.beta_b[r] = beta_b; o.delta_beta[r] = beta_b - beta_a;
}

// ---- regions -----------------------------------------------------------------------------------------------------------

struct RegIn {
  const int32_t *rname, *pos, *meth_a, *unmeth_a, *meth_b, *unmeth_b;
  const double *delta_beta, *p;
  uint32_t n;
  double max_p, min_delta;
  int32_t max_gap, min_sites;
};

// +1 / -1: row i is significant in that direction; 0: it is not (NaN compares false)
__device__ __forceinline__ int reg_dir(const RegIn &t, uint32_t i) {
  const double d = t.delta_beta[i];
  if (!(t.p[i] <= t.max_p) || !(fabs(d) >= t.min_delta) || !(d != 0.0)) return 0;
  return d > 0.0 ? 1 : -1;
}

// row i (i >= 1, significant in direction dir) continues the run of row i - 1
__device__ __forceinline__ bool reg_joins(const RegIn &t, uint32_t i, int dir) {
  return reg_dir(t, i - 1) == dir && t.rname[i - 1] == t.rname[i] && (int64_t)t.pos[i] - (int64_t)t.pos[i - 1] <= (int64_t)t.max_gap;
}

__global__ __launch_bounds__(CXC_WG) void k_reg_flag(RegIn t, uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * (uint32_t)CXC_WG + threadIdx.x;
  if (i >= t.n) return;
  const int dir = reg_dir(t, i);
  uint32_t f = 0;
  if (dir != 0 && !(i > 0 && reg_joins(t, i, dir))) {       // a run starts here: does it reach min_sites rows?
    uint32_t len = 1, j = i + 1;
    while (len < (uint32_t)t.min_sites && j < t.n && reg_dir(t, j) == dir && reg_joins(t, j, dir)) { len++; j++; }
    f = len >= (uint32_t)t.min_sites ? 1u : 0u;
  }
  flag[i] = f;
}

struct RegOut {
  int32_t *rname, *start, *end, *nsites, *direction;
  double *beta_a, *beta_b, *delta_beta, *mean_delta_beta, *p;
  uint32_t nregion;
};

__global__ __launch_bounds__(CXC_WG) void k_reg_emit(RegIn t, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ off, RegOut o) {
  const uint32_t i = blockIdx.x * (uint32_t)CXC_WG + threadIdx.x;
  if (i >= t.n || !flag[i]) return;
  const uint32_t r = off[i];
  if (r >= o.nregion) return;
  const int dir = reg_dir(t, i);
  int64_t ma = 0, ua = 0, mb = 0, ub = 0;
  double sum = 0.0;
  uint32_t j = i;
  do {                                                        // ascending rows
    ma += t.meth_a[j]; ua += t.unmeth_a[j]; mb += t.meth_b[j]; ub += t.unmeth_b[j];
    sum += t.delta_beta[j];
    j++;
  } while (j < t.n && reg_dir(t, j) == dir && reg_joins(t, j, dir));
  const uint32_t len = j - i;
  o.rname[r] = t.rname[i]; o.start[r] = t.pos[i]; o.end[r] = t.pos[j - 1]; o.nsites[r] = (int32_t)len; o.direction[r] = dir;
  const double beta_a = (double)ma / (double)(ma + ua), beta_b = (double)mb / (double)(mb + ub);
  o.beta_a[r] = beta_a; o.beta_b[r] = beta_b; o.delta_beta[r] = beta_b - beta_a;
  o.mean_delta_beta[r] = sum / (double)len;
  o.p[r] = fisher_cells(ma, ua, mb, ub);
}

// ---- host --------------------------------------------------------------------------------------------------------------

static int cx_compare(epi_engine *e, const CxTab &a, const CxTab &b, int32_t min_coverage, int32_t *const d_icols[8], double *const d_dcols[4],
                      int64_t cap, hipStream_t s, int64_t *ncommon_out, int64_t *nrow_out) {
  const char *who = "epi_cx_compare_dev";
  const int64_t na = a.n, nblk_a = (na + CXC_WG - 1) / CXC_WG, nblk_b = ((int64_t)b.n + CXC_WG - 1) / CXC_WG;
  EPI_TRY(check_grid(nblk_a, CXC_WG, "cytosine comparison site kernels"));
  EPI_TRY(check_grid(nblk_b, CXC_WG, "cytosine comparison site kernels"));
  CxKeepScratch w;                                            // keep flags, their scan, the matched rows of b
  EPI_TRY(w.take(na, 3));
  uint32_t *scal = w.scal;                                    // [0] a unsorted, [1] b unsorted, [2] common rows, [3] reported rows
  uint32_t *keep = w.flag, *off = keep + na, *brow = off + na;
  EPI_HIP(hipMemsetAsync(scal, 0, 64, s));
  prof_begin("cxcmp_match", s);
  hipLaunchKernelGGL(k_cxc_sorted, dim3((unsigned)nblk_a), dim3(CXC_WG), 0, s, a, &scal[0]);
  hipLaunchKernelGGL(k_cxc_sorted, dim3((unsigned)nblk_b), dim3(CXC_WG), 0, s, b, &scal[1]);
  hipLaunchKernelGGL(k_cxc_match, dim3((unsigned)nblk_a), dim3(CXC_WG), 0, s, a, b, min_coverage > 1 ? min_coverage : 1, keep, brow, &scal[2]);
  const int rc_scan = scan_exclusive_u32(keep, off, na, &scal[3], w.scan_tmp, s);
  prof_end("cxcmp_match", s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(rc_scan);
  uint32_t h[4];
  EPI_TRY(read_scalars(e, s, scal, sizeof(h), h));
  if (h[0] || h[1])
    return fail(EPI_ERR_ARG, "%s: the rows of the %s table are not strictly ascending in (rname, pos, strand)", who, h[0] ? "first" : "second");
  *ncommon_out = h[2];
  *nrow_out = h[3];
  EPI_TRY(cx_rows_fit(who, "rows", h[3], cap));
  if (h[3] == 0) return EPI_OK;
  EPI_TRY(cx_cols_arg(who, d_icols, 8, d_dcols, 4));
  CxcOut o;
  o.rname = d_icols[0]; o.strand = d_icols[1]; o.pos = d_icols[2]; o.context = d_icols[3];
  o.meth_a = d_icols[4]; o.unmeth_a = d_icols[5]; o.meth_b = d_icols[6]; o.unmeth_b = d_icols[7];
  o.beta_a = d_dcols[0]; o.beta_b = d_dcols[1]; o.delta_beta = d_dcols[2];
  o.nrow = h[3];
  prof_begin("cxcmp_emit", s);
  hipLaunchKernelGGL(k_cxc_emit, dim3((unsigned)nblk_a), dim3(CXC_WG), 0, s, a, b, keep, off, brow, o);
  prof_end("cxcmp_emit", s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(fisher_launch(o.meth_a, o.unmeth_a, o.meth_b, o.unmeth_b, (int64_t)h[3], d_dcols[3], s));
  EPI_HIP(hipStreamSynchronize(s));                           // (the scratch goes back when this returns)
  return EPI_OK;
}

static int cx_regions(epi_engine *e, const int32_t *const d_icols[8], const double *const d_dcols[4], int64_t n, double max_p,
                      double min_delta_beta, int32_t max_gap, int32_t min_sites, int32_t *const d_ricols[5], double *const d_rdcols[5],
                      int64_t cap, hipStream_t s, int64_t *nregion_out) {
  const char *who = "epi_cx_compare_regions_dev";
  const int64_t nblk = (n + CXC_WG - 1) / CXC_WG;
  EPI_TRY(check_grid(nblk, CXC_WG, "cytosine comparison region kernels"));
  CxKeepScratch w;
  EPI_TRY(w.take(n, 2));
  uint32_t *scal = w.scal, *flag = w.flag, *off = flag + n;
  RegIn t;
  t.rname = d_icols[0]; t.pos = d_icols[2];
  t.meth_a = d_icols[4]; t.unmeth_a = d_icols[5]; t.meth_b = d_icols[6]; t.unmeth_b = d_icols[7];
  t.delta_beta = d_dcols[2]; t.p = d_dcols[3];
  t.n = (uint32_t)n;
  t.max_p = max_p; t.min_delta = min_delta_beta; t.max_gap = max_gap; t.min_sites = min_sites;
  prof_begin("cxcmp_region_flag", s);
  hipLaunchKernelGGL(k_reg_flag, dim3((unsigned)nblk), dim3(CXC_WG), 0, s, t, flag);
  const int rc_scan = scan_exclusive_u32(flag, off, n, &scal[0], w.scan_tmp, s);
  prof_end("cxcmp_region_flag", s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(rc_scan);
  uint32_t h = 0;
  EPI_TRY(read_scalars(e, s, scal, sizeof(h), &h));
  *nregion_out = h;
  EPI_TRY(cx_rows_fit(who, "regions", h, cap));
  if (h == 0) return EPI_OK;
  EPI_TRY(cx_cols_arg(who, d_ricols, 5, d_rdcols, 5));
  RegOut o;
  o.rname = d_ricols[0]; o.start = d_ricols[1]; o.end = d_ricols[2]; o.nsites = d_ricols[3]; o.direction = d_ricols[4];
  o.beta_a = d_rdcols[0]; o.beta_b = d_rdcols[1]; o.delta_beta = d_rdcols[2]; o.mean_delta_beta = d_rdcols[3]; o.p = d_rdcols[4];
  o.nregion = h;
  prof_begin("cxcmp_region_emit", s);
  hipLaunchKernelGGL(k_reg_emit, dim3((unsigned)nblk), dim3(CXC_WG), 0, s, t, flag, off, o);
  prof_end("cxcmp_region_emit", s);
  EPI_HIP(hipGetLastError());
  EPI_HIP(hipStreamSynchronize(s));
  return EPI_OK;
}

}  // namespace epi

using namespace epi;

extern "C" {

int epi_fisher_exact_dev(epi_engine *e, const int32_t *d_a, const int32_t *d_b, const int32_t *d_c, const int32_t *d_d, int64_t n,
                         double *d_p, void *stream) {
  if (!e || n < 0 || (n > 0 && (!d_a || !d_b || !d_c || !d_d || !d_p))) return fail(EPI_ERR_ARG, "epi_fisher_exact_dev: bad arguments");
  if (n == 0) return EPI_OK;
  EPI_HIP(hipSetDevice(e->device));
  return fisher_launch(d_a, d_b, d_c, d_d, n, d_p, reinterpret_cast<hipStream_t>(stream));
}

int epi_cx_compare_dev(epi_engine *e, const int32_t *const d_a[6], int64_t na, const int32_t *const d_b[6], int64_t nb,
                       int32_t min_coverage, int32_t *const d_icols[8], double *const d_dcols[4], int64_t cap, void *stream,
                       int64_t *ncommon_out, int64_t *nrow_out) {
  const char *who = "epi_cx_compare_dev";
  if (!e || !ncommon_out || !nrow_out) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  *ncommon_out = 0; *nrow_out = 0;
  CxTab a, b;
  EPI_TRY(cx_tab_arg(who, d_a, na, kCxMaxRows, &a, cap));
  EPI_TRY(cx_tab_arg(who, d_b, nb, kCxMaxRows, &b));
  if (cap > 0 && (!d_icols || !d_dcols)) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  if (na == 0 || nb == 0) return EPI_OK;
  EPI_HIP(hipSetDevice(e->device));
  return cx_compare(e, a, b, min_coverage, d_icols, d_dcols, cap, reinterpret_cast<hipStream_t>(stream), ncommon_out, nrow_out);
}

int epi_cx_compare_regions_dev(epi_engine *e, const int32_t *const d_icols[8], const double *const d_dcols[4], int64_t n, double max_p,
                               double min_delta_beta, int32_t max_gap, int32_t min_sites, int32_t *const d_ricols[5],
                               double *const d_rdcols[5], int64_t cap, void *stream, int64_t *nregion_out) {
  const char *who = "epi_cx_compare_regions_dev";
  if (!e || !nregion_out) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  *nregion_out = 0;
  if (!(max_p >= 0.0 && max_p <= 1.0)) return fail(EPI_ERR_ARG, "%s: max_p = %g, a probability", who, max_p);
  if (!(min_delta_beta >= 0.0 && min_delta_beta <= 1.0)) return fail(EPI_ERR_ARG, "%s: min_delta_beta = %g, from 0 to 1", who, min_delta_beta);
  if (max_gap < 0) return fail(EPI_ERR_ARG, "%s: negative max_gap", who);
  if (min_sites < 1) return fail(EPI_ERR_ARG, "%s: min_sites = %d, regions hold at least one site", who, min_sites);
  EPI_TRY(cx_rows_arg(who, n, kCxMaxRows, cap));
  if (cap > 0 && (!d_ricols || !d_rdcols)) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  if (n == 0) return EPI_OK;
  EPI_TRY(cx_cols_arg(who, d_icols, 8, d_dcols, 4));
  EPI_HIP(hipSetDevice(e->device));
  return cx_regions(e, d_icols, d_dcols, n, max_p, min_delta_beta, max_gap, min_sites, d_ricols, d_rdcols, cap,
                    reinterpret_cast<hipStream_t>(stream), nregion_out);
}

}  // extern "C"
