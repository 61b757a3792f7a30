// Multiple-testing correction of a column of p-values (include/epihip.h, epi_p_adjust_dev, has the definitions).  No
// reference interface is replaced.  The call is stateless: it reads and writes the caller's columns, takes its scratch for
// the length of the call and touches no batch.  All on the call's stream:
//  Keys     k_padj_keys: a row's key is the bit pattern of p + 0.0 (ascending as u64 exactly as the doubles ascend on
//           [0, 1]; NaN: ~0, behind everything), its value the row.  The same pass ORs the range flag, counts the valid
//           rows (one add per wave) and fills the histograms of all eight key bytes (per workgroup in LDS, then one add per
//           occupied bin); k_padj_plan marks the bytes in which every key agrees: their passes are skipped.
//  Sort     least significant byte first, per byte that is left: radix_sort.hip's stable LSD sort, in a SortPairs workspace
//           (radix_sort.hpp) that is one piece of the call's arena.
//  Terms   k_padj_terms: t_r of the method, in the header's operation order, from the sorted keys; then a device-wide
//           inclusive scan of doubles under min or max (scan.hpp's three launches; min and max are exact and associative,
//           so no launch shape enters a result), walking the ranks downwards for the suffix minimum.
//  Scatter  k_padj_scatter: q[order[r]] = min(1, t_r), NaN for the ranks of the NaN rows; order[r] to the caller.
#include "radix_sort.hpp"

namespace epi {

constexpr int PADJ_WG = 256;
constexpr int PADJ_KEY_ITEMS = 8;                              // rows per thread of k_padj_keys
constexpr int PADJ_KEY_TILE = PADJ_WG * PADJ_KEY_ITEMS;
constexpr int DSCAN_ITEMS = 4;                                 // consecutive terms per thread of the double scan
constexpr int DSCAN_BLOCK = PADJ_WG * DSCAN_ITEMS;
constexpr uint64_t PADJ_NAN_KEY = ~0ull;

struct PadjScalars {                   // 64 bytes in front of the eight global byte histograms
  uint32_t bad;                        // some value is neither NaN nor in [0, 1]
  uint32_t nvalid;                     // rows that are not NaN
  uint32_t skip[8];                    // every key has the same byte d: pass d moves nothing
  uint32_t unused[6];
};
static_assert(sizeof(PadjScalars) == 64, "PadjScalars layout");

// ---- keys ----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(PADJ_WG) void k_padj_keys(const double *__restrict__ p, uint32_t n, uint64_t *__restrict__ key,
                                                       uint32_t *__restrict__ row, PadjScalars *__restrict__ sc,
                                                       uint32_t *__restrict__ ghist /* [8][256] */) {
  __shared__ uint32_t s_hist[8 * 256];
  for (int i = threadIdx.x; i < 8 * 256; i += PADJ_WG) s_hist[i] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)PADJ_KEY_TILE;                 // (n < 2^31: no wrap)
  uint32_t nvalid = 0;
  bool bad = false;
#pragma unroll
  for (int i = 0; i < PADJ_KEY_ITEMS; i++) {
    const uint32_t r = base + (uint32_t)i * PADJ_WG + threadIdx.x;
    const bool active = r < n;
    uint64_t k = PADJ_NAN_KEY;
    if (active) {
      const double v = p[r];
      if (v == v) {
        const double x = v + 0.0;                                             // -0.0 -> 0.0
        k = (uint64_t)__double_as_longlong(x);
        nvalid++;
        if (!(x >= 0.0 && x <= 1.0)) bad = true;
      }
      key[r] = k;
      row[r] = r;
    }
    const uint64_t amask = __ballot(active);
#pragma unroll
    for (int d = 0; d < 8; d++) hist_add(&s_hist[d * 256], (uint32_t)(k >> (8 * d)) & 255u, active, amask);
  }
  const uint32_t wsum = wave_sum_u32(nvalid);
  const bool wbad = __any(bad);
  if ((threadIdx.x & 63) == 0) {
    if (wsum) atomicAdd(&sc->nvalid, wsum);
    if (wbad) atomicOr(&sc->bad, 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 8 * 256; i += PADJ_WG) {
    const uint32_t c = s_hist[i];
    if (c) atomicAdd(&ghist[i], c);
  }
}

// one workgroup: byte d is skipped when at most one of its 256 bins is occupied
__global__ __launch_bounds__(PADJ_WG) void k_padj_plan(const uint32_t *__restrict__ ghist, PadjScalars *__restrict__ sc) {
  for (int d = 0; d < 8; d++) {
    const int occupied = __syncthreads_count(ghist[d * 256 + threadIdx.x] != 0u);
    if (threadIdx.x == 0) sc->skip[d] = occupied <= 1 ? 1u : 0u;
  }
}

// ---- terms -----------------------------------------------------------------------------------------------------------------

struct PadjTerms {
  int32_t method;
  uint32_t m;                          // valid rows: ranks 1 .. m
  int64_t N;                           // tests adjusted for
  double c;                            // BY: sum of 1 / k over k = 1 .. N
};

__global__ __launch_bounds__(PADJ_WG) void k_padj_terms(const uint64_t *__restrict__ key, PadjTerms a, double *__restrict__ t) {
  const uint32_t r = blockIdx.x * (uint32_t)PADJ_WG + threadIdx.x;
  if (r >= a.m) return;
  const double s = __longlong_as_double((long long)key[r]);
  const double N = (double)a.N, j = (double)(r + 1u);
  double x;
  switch (a.method) {
    case EPI_PADJ_BONFERRONI: x = N * s; break;
    case EPI_PADJ_HOLM:
    case EPI_PADJ_HOCHBERG: x = (double)(a.N + 1 - (int64_t)(r + 1u)) * s; break;
    case EPI_PADJ_BH: x = (N / j) * s; break;
    case EPI_PADJ_BY: x = ((a.c * N) / j) * s; break;
    default: x = s; break;
  }
  t[r] = x;
}

// ---- inclusive scan of doubles under min or max ------------------------------------------------------------------------------
// In place (scan.hpp: an element is loaded and stored by the same thread).  Element L of the scan is t[L], or t[m - 1 - L] when
// `rev` (a suffix scan): reversal is the functor's business, not the scan's.  k_padj_terms writes finite terms >= +0.0 (p in
// [0, 1] after the range check, N and c finite and positive): no NaN and no -0.0, so min and max are exact and order-free.
struct PadjTermRef {
  double *t;
  uint32_t m;
  bool rev;
  __device__ double &at(int64_t L) const { return t[rev ? (int64_t)m - 1 - L : L]; }
  __device__ double operator()(int64_t L) const { return at(L); }
  __device__ void operator()(int64_t L, double, double inclusive) const { at(L) = inclusive; }
};

template <bool MAX> static int dscan_inclusive(double *t, uint32_t m, bool rev, DevBuf &tmp, hipStream_t s) {
  using Op = MinMaxF64<MAX>;
  const PadjTermRef ref{t, m, rev};
  return device_scan<Op, DSCAN_ITEMS, PADJ_WG>((int64_t)m, ref, ref, Op::identity(), nullptr, tmp, s);
}

// ---- scatter ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(PADJ_WG) void k_padj_scatter(const uint32_t *__restrict__ row, const double *__restrict__ t, uint32_t n,
                                                          uint32_t m, double *__restrict__ q, int32_t *__restrict__ order) {
  const uint32_t r = blockIdx.x * (uint32_t)PADJ_WG + threadIdx.x;
  if (r >= n) return;
  const uint32_t i = row[r];
  if (i >= n) return;
  double x = __builtin_nan("");
  if (r < m) { x = t[r]; x = x < 1.0 ? x : 1.0; }
  q[i] = x;
  if (order) order[r] = (int32_t)i;
}

// ---- host ------------------------------------------------------------------------------------------------------------------

static int p_adjust(epi_engine *e, const double *d_p, int64_t n, int32_t method, int64_t n_tests, double *d_q, int32_t *d_order,
                    hipStream_t s, int64_t *nvalid_out) {
  const char *who = "epi_p_adjust_dev";
  const uint32_t un = (uint32_t)n;
  const int64_t nblk_key = (n + PADJ_KEY_TILE - 1) / PADJ_KEY_TILE, nblk_row = (n + PADJ_WG - 1) / PADJ_WG;
  const int64_t nblk_scan = ((int64_t)SortPairs::table_words((size_t)n) + 4095) / 4096, nblk_dscan = (n + DSCAN_BLOCK - 1) / DSCAN_BLOCK;
  EPI_TRY(check_grid(nblk_row, PADJ_WG, "p-value adjustment kernels"));
  ScratchArena w;                                             // every piece rounded to 256 bytes
  const size_t o_scal = w.reserve(sizeof(PadjScalars) + 8 * 256 * 4, 256), o_sort = w.reserve(SortPairs::bytes((size_t)n), 256);
  const size_t o_terms = w.reserve((size_t)n * 8, 256), o_scan = w.reserve((size_t)nblk_scan * 4, 256), o_agg = w.reserve((size_t)nblk_dscan * 8, 256);
  EPI_TRY(w.alloc());
  PadjScalars *sc; uint64_t *sort_mem; double *terms, *agg_mem; uint32_t *scan_mem;
  EPI_TRY(w.at(o_scal, &sc)); EPI_TRY(w.at(o_sort, &sort_mem)); EPI_TRY(w.at(o_terms, &terms)); EPI_TRY(w.at(o_scan, &scan_mem)); EPI_TRY(w.at(o_agg, &agg_mem));
  SortPairs sort(sort_mem, (size_t)n);
  DevBuf scan_tmp = DevBuf::view(scan_mem, (size_t)nblk_scan * 4), agg = DevBuf::view(agg_mem, (size_t)nblk_dscan * 8);
  uint32_t *ghist = reinterpret_cast<uint32_t *>(sc + 1);
  EPI_HIP(hipMemsetAsync(sc, 0, sizeof(PadjScalars) + 8 * 256 * 4, s));
  prof_begin("padj_keys", s);
  hipLaunchKernelGGL(k_padj_keys, dim3((unsigned)nblk_key), dim3(PADJ_WG), 0, s, d_p, un, sort.keys_in(), sort.vals_in(), sc, ghist);
  hipLaunchKernelGGL(k_padj_plan, dim3(1), dim3(PADJ_WG), 0, s, ghist, sc);
  prof_end("padj_keys", s);
  EPI_HIP(hipGetLastError());
  PadjScalars h;
  EPI_TRY(read_scalars(e, s, sc, sizeof(PadjScalars), &h));
  if (h.bad) return fail(EPI_ERR_ARG, "%s: a p-value is neither NA nor in [0, 1]", who);
  const int64_t m = h.nvalid;
  *nvalid_out = m;
  if (n_tests > 0 && n_tests < m) return fail(EPI_ERR_ARG, "%s: n_tests = %lld, below the %lld p-values that are not NA", who, (long long)n_tests, (long long)m);
  const int64_t N = n_tests > 0 ? n_tests : m;

  uint32_t bytes = 0;
  for (int d = 0; d < 8; d++) if (!h.skip[d]) bytes |= 1u << d;
  EPI_TRY(sort.sort(bytes, scan_tmp, s));

  const uint32_t um = (uint32_t)m;
  if (m > 0) {
    PadjTerms a;
    a.method = method; a.m = um; a.N = N; a.c = 0.0;
    if (method == EPI_PADJ_BY)
      for (int64_t k = 1; k <= N; k++) a.c += 1.0 / (double)k;
    prof_begin("padj_terms", s);
    hipLaunchKernelGGL(k_padj_terms, dim3((um + PADJ_WG - 1) / PADJ_WG), dim3(PADJ_WG), 0, s, sort.keys(), a, terms);
    prof_end("padj_terms", s);
    int rc = EPI_OK;
    prof_begin("padj_dscan", s);
    if (method == EPI_PADJ_HOLM) rc = dscan_inclusive<true>(terms, um, false, agg, s);
    else if (method == EPI_PADJ_HOCHBERG || method == EPI_PADJ_BH || method == EPI_PADJ_BY) rc = dscan_inclusive<false>(terms, um, true, agg, s);
    prof_end("padj_dscan", s);
    EPI_HIP(hipGetLastError());
    EPI_TRY(rc);
  }
  prof_begin("padj_scatter", s);
  hipLaunchKernelGGL(k_padj_scatter, dim3((unsigned)nblk_row), dim3(PADJ_WG), 0, s, sort.vals(), terms, un, um, d_q, d_order);
  prof_end("padj_scatter", s);
  EPI_HIP(hipGetLastError());
  EPI_HIP(hipStreamSynchronize(s));                           // (the scratch goes back when this returns)
  return EPI_OK;
}

}  // namespace epi

using namespace epi;

extern "C" {

int epi_p_adjust_dev(epi_engine *e, const double *d_p, int64_t n, int32_t method, int64_t n_tests, double *d_q, int32_t *d_order, void *stream,
                     int64_t *nvalid_out) {
  const char *who = "epi_p_adjust_dev";
  if (!e || !nvalid_out) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  *nvalid_out = 0;
  if (method < EPI_PADJ_NONE || method > EPI_PADJ_BY) return fail(EPI_ERR_ARG, "%s: method %d, one of EPI_PADJ_*", who, method);
  if (n < 0) return fail(EPI_ERR_ARG, "%s: negative row count", who);
  if (n >= (1LL << 31) || n_tests >= (1LL << 31)) return fail(EPI_ERR_ARG, "%s: %lld rows, n_tests = %lld", who, (long long)n, (long long)n_tests);
  if (n > 0 && (!d_p || !d_q)) return fail(EPI_ERR_ARG, "%s: NULL column", who);
  if (n == 0) return EPI_OK;
  EPI_HIP(hipSetDevice(e->device));
  return p_adjust(e, d_p, n, method, n_tests, d_q, d_order, reinterpret_cast<hipStream_t>(stream), nvalid_out);
}

}  // extern "C"
