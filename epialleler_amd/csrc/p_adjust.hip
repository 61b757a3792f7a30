// Multiple-testing correction of a column of p-values (include/epihip.h, epi_p_adjust_dev, has the definitions).  No
// reference interface is replaced.  The call is stateless: it reads and writes the caller's columns, takes its scratch for
// the length of the call and touches no batch.  All on the call's stream:
//  Keys     k_padj_keys: a row's key is the bit pattern of p + 0.0 (ascending as u64 exactly as the doubles ascend on
//           [0, 1]; NaN: ~0, behind everything), its value the row.  The same pass ORs the range flag, counts the valid
//           rows (one add per wave) and fills the histograms of all eight key bytes (per workgroup in LDS, then one add per
//           occupied bin); k_padj_plan marks the bytes in which every key agrees: their passes are skipped.
//  Sort     least significant byte first, per byte that is left: k_padj_hist (a workgroup's tile of 4096 keys -> its column of
//           the [digit][workgroup] table), util.hip's scan over the table, k_padj_sort_scatter.  The scatter is STABLE: a
//           wave owns 1024 consecutive keys of the tile and takes them 64 at a time; a key's rank among the wave's equal
//           digits is the wave's running count of that digit (one lane per digit stores it, plain LDS stores) plus the
//           number of lower lanes of the match mask (eight ballots).  No rank comes from what an LDS atomic returns.  The
//           tile is put into digit order in LDS (keys, then rows, in one 32 KB buffer) and stored from there, so that a
//           wave's stores run along the digits' runs instead of 64 ways apart.  The per-byte launch sequence is
//           radix_sort_pairs (common.hpp), which the FDRP report's site -> rows index (fdrp.hip) calls as well.
//  Terms   k_padj_terms: t_r of the method, in the header's operation order, from the sorted keys; then a device-wide
//           inclusive scan of doubles under min or max (k_dscan_reduce, k_dscan_carry, k_dscan_apply: reduce-then-scan as
//           util.hip's three launches; min and max are exact and associative, so no launch shape enters a result), walking
//           the ranks downwards for the suffix minimum.
//  Scatter  k_padj_scatter: q[order[r]] = min(1, t_r), NaN for the ranks of the NaN rows; order[r] to the caller.
#include <string.h>
#include "common.hpp"

namespace epi {

constexpr int PADJ_WG = 256;
constexpr int PADJ_WAVES = PADJ_WG / 64;
constexpr int PADJ_KEY_ITEMS = 8;                              // rows per thread of k_padj_keys
constexpr int PADJ_KEY_TILE = PADJ_WG * PADJ_KEY_ITEMS;
constexpr int PADJ_SORT_ITEMS = 16;                            // keys per thread of a sorting pass
constexpr int PADJ_WAVE_KEYS = 64 * PADJ_SORT_ITEMS;           // consecutive keys a wave owns
constexpr int PADJ_SORT_TILE = PADJ_WG * PADJ_SORT_ITEMS;      // 4096 keys per workgroup
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

// one LDS add per lane, or one per wave when every active lane holds the same bin (the exponent bytes of a p-value column)
__device__ __forceinline__ void hist_add(uint32_t *hist, uint32_t bin, bool active, uint64_t amask) {
  if (amask == 0) return;                                                     // (uniform)
  const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)bin, __ffsll((unsigned long long)amask) - 1);
  if (__all(!active || bin == first)) {
    if ((threadIdx.x & 63) == 0) atomicAdd(&hist[first], (uint32_t)__popcll(amask));
  } else if (active) {
    atomicAdd(&hist[bin], 1u);
  }
}

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

// ---- one pass of the sort --------------------------------------------------------------------------------------------------

// table[digit * nblk + workgroup] = keys of the workgroup's tile with that digit
__global__ __launch_bounds__(PADJ_WG) void k_padj_hist(const uint64_t *__restrict__ key, uint32_t n, int shift, uint32_t nblk,
                                                       uint32_t *__restrict__ table) {
  __shared__ uint32_t s_hist[256];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)PADJ_SORT_TILE + (threadIdx.x >> 6) * (uint32_t)PADJ_WAVE_KEYS + (threadIdx.x & 63);
#pragma unroll
  for (int i = 0; i < PADJ_SORT_ITEMS; i++) {
    const uint32_t r = base + (uint32_t)i * 64u;
    const bool active = r < n;
    const uint32_t d = active ? (uint32_t)(key[r] >> shift) & 255u : 0u;
    hist_add(s_hist, d, active, __ballot(active));
  }
  __syncthreads();
  table[(size_t)threadIdx.x * nblk + blockIdx.x] = s_hist[threadIdx.x];
}

// off[digit * nblk + workgroup]: the exclusive scan of the table = where the workgroup's first key of that digit goes
__global__ __launch_bounds__(PADJ_WG) void k_padj_sort_scatter(const uint64_t *__restrict__ key_in, const uint32_t *__restrict__ row_in,
                                                               uint32_t n, int shift, uint32_t nblk, const uint32_t *__restrict__ off,
                                                               uint64_t *__restrict__ key_out, uint32_t *__restrict__ row_out) {
  __shared__ uint32_t s_cnt[PADJ_WAVES][256];       // per wave: keys of a digit seen so far; then: where in the tile its next key of the digit goes
  __shared__ uint64_t s_stage[PADJ_SORT_TILE];      // the tile's keys in digit order; then, as u32, its rows
  __shared__ uint32_t s_goff[256], s_wsum[PADJ_WAVES];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int w = 0; w < PADJ_WAVES; w++) s_cnt[w][threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)PADJ_SORT_TILE + wave * (uint32_t)PADJ_WAVE_KEYS + lane;
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t k[PADJ_SORT_ITEMS];
  uint32_t v[PADJ_SORT_ITEMS], rank[PADJ_SORT_ITEMS];
#pragma unroll
  for (int i = 0; i < PADJ_SORT_ITEMS; i++) {
    const uint32_t r = base + (uint32_t)i * 64u;
    const bool active = r < n;
    k[i] = active ? key_in[r] : 0ull;
    v[i] = active ? row_in[r] : 0u;
  }
#pragma unroll
  for (int i = 0; i < PADJ_SORT_ITEMS; i++) {
    const bool active = base + (uint32_t)i * 64u < n;
    const uint32_t d = (uint32_t)(k[i] >> shift) & 255u;
    uint64_t same = __ballot(active);                                         // the active lanes that hold this lane's digit
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const bool bit = (d >> b) & 1u;
      const uint64_t bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    const uint32_t seen = s_cnt[wave][d];
    rank[i] = seen + (uint32_t)__popcll(same & below);
    __builtin_amdgcn_wave_barrier();                                          // every lane has read before one lane per digit writes
    if (active && (same >> lane) == 1ull) s_cnt[wave][d] = rank[i] + 1u;      // the highest lane of the set: seen + |set|
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {                                                 // thread = digit: where the tile's run of the digit starts, the waves' shares in wave order
    const uint32_t d = threadIdx.x;
    uint32_t c[PADJ_WAVES], total = 0;
    for (int w = 0; w < PADJ_WAVES; w++) { c[w] = s_cnt[w][d]; total += c[w]; }
    const uint32_t inc = wave_scan_u32(total);
    if (lane == 63) s_wsum[wave] = inc;
    __syncthreads();
    uint32_t start = inc - total;
    for (uint32_t w = 0; w < wave; w++) start += s_wsum[w];
    s_goff[d] = off[(size_t)d * nblk + blockIdx.x] - start;                   // (mod 2^32) + a key's place in the tile = its place in the output
    uint32_t at = start;
    for (int w = 0; w < PADJ_WAVES; w++) { s_cnt[w][d] = at; at += c[w]; }
  }
  __syncthreads();
  // the tile in digit order through LDS, so that a wave's stores run along the digits' runs: first the keys, then the rows
#pragma unroll
  for (int i = 0; i < PADJ_SORT_ITEMS; i++) {
    const bool active = base + (uint32_t)i * 64u < n;
    rank[i] += s_cnt[wave][(uint32_t)(k[i] >> shift) & 255u];                 // the key's place in the tile
    if (active && rank[i] < (uint32_t)PADJ_SORT_TILE) s_stage[rank[i]] = k[i];
  }
  __syncthreads();
  const uint32_t tile0 = blockIdx.x * (uint32_t)PADJ_SORT_TILE;
  const uint32_t count = n - tile0 < (uint32_t)PADJ_SORT_TILE ? n - tile0 : (uint32_t)PADJ_SORT_TILE;
  uint32_t dst[PADJ_SORT_ITEMS];
#pragma unroll
  for (int i = 0; i < PADJ_SORT_ITEMS; i++) {
    const uint32_t j = (uint32_t)i * PADJ_WG + threadIdx.x;
    dst[i] = n;
    if (j < count) {
      const uint64_t kk = s_stage[j];
      dst[i] = s_goff[(uint32_t)(kk >> shift) & 255u] + j;
      if (dst[i] < n) key_out[dst[i]] = kk;
    }
  }
  __syncthreads();
  uint32_t *s_rows = reinterpret_cast<uint32_t *>(s_stage);
#pragma unroll
  for (int i = 0; i < PADJ_SORT_ITEMS; i++) {
    const bool active = base + (uint32_t)i * 64u < n;
    if (active && rank[i] < (uint32_t)PADJ_SORT_TILE) s_rows[rank[i]] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PADJ_SORT_ITEMS; i++) {
    const uint32_t j = (uint32_t)i * PADJ_WG + threadIdx.x;
    if (j < count && dst[i] < n) row_out[dst[i]] = s_rows[j];
  }
}

int64_t radix_sort_blocks(int64_t n) { return (n + PADJ_SORT_TILE - 1) / PADJ_SORT_TILE; }

int radix_sort_pairs(uint64_t *const key[2], uint32_t *const row[2], uint32_t n, uint32_t bytes, uint32_t *table, uint32_t *off,
                     DevBuf &scan_tmp, hipStream_t s, int *cur_out) {
  const int64_t nblk = radix_sort_blocks((int64_t)n);
  int cur = 0;
  for (int d = 0; d < 8; d++) {
    if (!((bytes >> d) & 1u)) continue;
    prof_begin("padj_hist", s);
    hipLaunchKernelGGL(k_padj_hist, dim3((unsigned)nblk), dim3(PADJ_WG), 0, s, key[cur], n, 8 * d, (uint32_t)nblk, table);
    prof_end("padj_hist", s);
    prof_begin("padj_table_scan", s);
    const int rc = scan_exclusive_u32(table, off, nblk * 256, nullptr, scan_tmp, s);
    prof_end("padj_table_scan", s);
    EPI_TRY(rc);
    prof_begin("padj_sort_scatter", s);
    hipLaunchKernelGGL(k_padj_sort_scatter, dim3((unsigned)nblk), dim3(PADJ_WG), 0, s, key[cur], row[cur], n, 8 * d, (uint32_t)nblk,
                       off, key[cur ^ 1], row[cur ^ 1]);
    prof_end("padj_sort_scatter", s);
    cur ^= 1;
  }
  EPI_HIP(hipGetLastError());
  *cur_out = cur;
  return EPI_OK;
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
// Logical element L of the scan is t[L], or t[m - 1 - L] when `rev` (a suffix scan).  A workgroup owns DSCAN_BLOCK logical
// elements, a thread DSCAN_ITEMS consecutive ones.

template <bool MAX> __device__ __forceinline__ double dscan_op(double a, double b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); }
template <bool MAX> __device__ __forceinline__ double dscan_identity() { return MAX ? -__builtin_inf() : __builtin_inf(); }

// inclusive scan of one value per thread across the workgroup; *total = the workgroup's aggregate
template <bool MAX> __device__ __forceinline__ double dscan_block(double v, double *total, double *s_wave /* [PADJ_WAVES] */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(v, d, 64);
    if (lane >= d) v = dscan_op<MAX>(o, v);
  }
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  double before = dscan_identity<MAX>(), all = dscan_identity<MAX>();
  for (int w = 0; w < PADJ_WAVES; w++) {
    const double x = s_wave[w];
    if (w < wave) before = dscan_op<MAX>(before, x);
    all = dscan_op<MAX>(all, x);
  }
  __syncthreads();
  *total = all;
  return dscan_op<MAX>(before, v);
}

template <bool MAX> __global__ __launch_bounds__(PADJ_WG) void k_dscan_reduce(const double *__restrict__ t, uint32_t m, int rev,
                                                                              double *__restrict__ agg) {
  __shared__ double s_wave[PADJ_WAVES];
  const uint32_t base = blockIdx.x * (uint32_t)DSCAN_BLOCK + threadIdx.x * (uint32_t)DSCAN_ITEMS;
  double acc = dscan_identity<MAX>();
#pragma unroll
  for (int i = 0; i < DSCAN_ITEMS; i++) {
    const uint32_t L = base + (uint32_t)i;
    if (L < m) acc = dscan_op<MAX>(acc, t[rev ? m - 1u - L : L]);
  }
  double total;
  (void)dscan_block<MAX>(acc, &total, s_wave);
  if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// one workgroup: agg[k] <- the aggregate of everything in front of workgroup k (the identity for k = 0)
template <bool MAX> __global__ __launch_bounds__(PADJ_WG) void k_dscan_carry(double *__restrict__ agg, uint32_t nb) {
  __shared__ double s_wave[PADJ_WAVES], s_last[PADJ_WAVES];
  double carry = dscan_identity<MAX>();
  for (uint32_t base = 0; base < nb; base += PADJ_WG) {
    const uint32_t k = base + threadIdx.x;
    const double v = k < nb ? agg[k] : dscan_identity<MAX>();
    double total;
    const double inc = dscan_block<MAX>(v, &total, s_wave);
    const double prev = __shfl_up(inc, 1, 64);                                // exclusive = the inclusive value of the thread before
    if ((threadIdx.x & 63) == 63) s_last[threadIdx.x >> 6] = inc;
    __syncthreads();
    double ex = carry;
    if ((threadIdx.x & 63) != 0) ex = dscan_op<MAX>(carry, prev);
    else if (threadIdx.x != 0) ex = dscan_op<MAX>(carry, s_last[(threadIdx.x >> 6) - 1]);
    if (k < nb) agg[k] = ex;
    carry = dscan_op<MAX>(carry, total);
    __syncthreads();
  }
}

template <bool MAX> __global__ __launch_bounds__(PADJ_WG) void k_dscan_apply(double *__restrict__ t, uint32_t m, int rev,
                                                                             const double *__restrict__ agg) {
  __shared__ double s_wave[PADJ_WAVES], s_last[PADJ_WAVES];
  const uint32_t base = blockIdx.x * (uint32_t)DSCAN_BLOCK + threadIdx.x * (uint32_t)DSCAN_ITEMS;
  double x[DSCAN_ITEMS];
  double acc = dscan_identity<MAX>();
#pragma unroll
  for (int i = 0; i < DSCAN_ITEMS; i++) {
    const uint32_t L = base + (uint32_t)i;
    x[i] = L < m ? t[rev ? m - 1u - L : L] : dscan_identity<MAX>();
    acc = dscan_op<MAX>(acc, x[i]);
    x[i] = acc;                                                               // inclusive within the thread
  }
  double total;
  const double inc = dscan_block<MAX>(acc, &total, s_wave);                   // inclusive over the threads' aggregates
  // what lies in front of this thread: the workgroups before, and the threads before in this workgroup
  const double prev = __shfl_up(inc, 1, 64);
  if ((threadIdx.x & 63) == 63) s_last[threadIdx.x >> 6] = inc;
  __syncthreads();
  double front = agg[blockIdx.x];
  if ((threadIdx.x & 63) != 0) front = dscan_op<MAX>(front, prev);
  else if (threadIdx.x != 0) front = dscan_op<MAX>(front, s_last[(threadIdx.x >> 6) - 1]);
#pragma unroll
  for (int i = 0; i < DSCAN_ITEMS; i++) {
    const uint32_t L = base + (uint32_t)i;
    if (L < m) t[rev ? m - 1u - L : L] = dscan_op<MAX>(front, x[i]);
  }
}

template <bool MAX> static int dscan_inclusive(double *t, uint32_t m, bool rev, DevBuf &tmp, hipStream_t s) {
  if (m == 0) return EPI_OK;
  const uint32_t nb = (m + DSCAN_BLOCK - 1) / DSCAN_BLOCK;
  EPI_TRY(tmp.ensure((size_t)nb * 8));
  double *agg = tmp.as<double>();
  hipLaunchKernelGGL(k_dscan_reduce<MAX>, dim3(nb), dim3(PADJ_WG), 0, s, t, m, rev ? 1 : 0, agg);
  hipLaunchKernelGGL(k_dscan_carry<MAX>, dim3(1), dim3(PADJ_WG), 0, s, agg, nb);
  hipLaunchKernelGGL(k_dscan_apply<MAX>, dim3(nb), dim3(PADJ_WG), 0, s, t, m, rev ? 1 : 0, agg);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
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

struct PadjScratch {                    // one allocation, released when the call returns; the buffers are pieces of it
  DevBuf arena;
  size_t used = 0;
  size_t reserve(size_t bytes) { const size_t at = used; used += (bytes + 255) & ~(size_t)255; return at; }
  template <class T> T *at(size_t off) const { return reinterpret_cast<T *>(arena.as<char>() + off); }
};

static int p_adjust(epi_engine *e, const double *d_p, int64_t n, int32_t method, int64_t n_tests, double *d_q, int32_t *d_order,
                    hipStream_t s, int64_t *nvalid_out) {
  const char *who = "epi_p_adjust_dev";
  const uint32_t un = (uint32_t)n;
  const int64_t nblk_key = (n + PADJ_KEY_TILE - 1) / PADJ_KEY_TILE, nblk_sort = (n + PADJ_SORT_TILE - 1) / PADJ_SORT_TILE;
  const int64_t nblk_row = (n + PADJ_WG - 1) / PADJ_WG, nblk_scan = (nblk_sort * 256 + 4095) / 4096, nblk_dscan = (n + DSCAN_BLOCK - 1) / DSCAN_BLOCK;
  EPI_TRY(check_grid(nblk_row, PADJ_WG, "p-value adjustment kernels"));
  PadjScratch w;
  const size_t o_scal = w.reserve(sizeof(PadjScalars) + 8 * 256 * 4);
  const size_t o_key[2] = {w.reserve((size_t)n * 8), w.reserve((size_t)n * 8)}, o_row[2] = {w.reserve((size_t)n * 4), w.reserve((size_t)n * 4)};
  const size_t o_terms = w.reserve((size_t)n * 8), o_table = w.reserve((size_t)nblk_sort * 256 * 4), o_off = w.reserve((size_t)nblk_sort * 256 * 4);
  const size_t o_scan = w.reserve((size_t)nblk_scan * 4), o_agg = w.reserve((size_t)nblk_dscan * 8);
  EPI_TRY(w.arena.ensure(w.used));
  uint64_t *const key[2] = {w.at<uint64_t>(o_key[0]), w.at<uint64_t>(o_key[1])};
  uint32_t *const row[2] = {w.at<uint32_t>(o_row[0]), w.at<uint32_t>(o_row[1])};
  double *const terms = w.at<double>(o_terms);
  uint32_t *const table = w.at<uint32_t>(o_table), *const off = w.at<uint32_t>(o_off);
  DevBuf scan_tmp = DevBuf::view(w.at<void>(o_scan), (size_t)nblk_scan * 4), agg = DevBuf::view(w.at<void>(o_agg), (size_t)nblk_dscan * 8);
  PadjScalars *sc = w.at<PadjScalars>(o_scal);
  uint32_t *ghist = reinterpret_cast<uint32_t *>(sc + 1);
  EPI_HIP(hipMemsetAsync(sc, 0, sizeof(PadjScalars) + 8 * 256 * 4, s));
  prof_begin("padj_keys", s);
  hipLaunchKernelGGL(k_padj_keys, dim3((unsigned)nblk_key), dim3(PADJ_WG), 0, s, d_p, un, key[0], row[0], sc, ghist);
  hipLaunchKernelGGL(k_padj_plan, dim3(1), dim3(PADJ_WG), 0, s, ghist, sc);
  prof_end("padj_keys", s);
  EPI_HIP(hipGetLastError());
  PadjScalars h;
  EPI_HIP(hipMemcpyAsync(e->h_scalars, sc, sizeof(PadjScalars), hipMemcpyDeviceToHost, s));
  EPI_HIP(hipStreamSynchronize(s));
  memcpy(&h, e->h_scalars, sizeof(PadjScalars));
  if (h.bad) return fail(EPI_ERR_ARG, "%s: a p-value is neither NA nor in [0, 1]", who);
  const int64_t m = h.nvalid;
  *nvalid_out = m;
  if (n_tests > 0 && n_tests < m) return fail(EPI_ERR_ARG, "%s: n_tests = %lld, below the %lld p-values that are not NA", who, (long long)n_tests, (long long)m);
  const int64_t N = n_tests > 0 ? n_tests : m;

  uint32_t bytes = 0;
  for (int d = 0; d < 8; d++) if (!h.skip[d]) bytes |= 1u << d;
  int cur = 0;
  EPI_TRY(radix_sort_pairs(key, row, un, bytes, table, off, scan_tmp, s, &cur));

  const uint32_t um = (uint32_t)m;
  if (m > 0) {
    PadjTerms a;
    a.method = method; a.m = um; a.N = N; a.c = 0.0;
    if (method == EPI_PADJ_BY)
      for (int64_t k = 1; k <= N; k++) a.c += 1.0 / (double)k;
    prof_begin("padj_terms", s);
    hipLaunchKernelGGL(k_padj_terms, dim3((um + PADJ_WG - 1) / PADJ_WG), dim3(PADJ_WG), 0, s, key[cur], a, terms);
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
  hipLaunchKernelGGL(k_padj_scatter, dim3((unsigned)nblk_row), dim3(PADJ_WG), 0, s, row[cur], terms, un, um, d_q, d_order);
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
