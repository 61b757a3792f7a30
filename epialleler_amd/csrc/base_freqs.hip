// rcpp_get_base_freqs (src/rcpp_get_base_freqs.cpp:15-57; caller .getBaseFreqReport, R/internal.R:611-676): for every
// read x and every VCF site i on the read's rname inside [start, start + len - 1], one count in column
//   seq_nt16_int[byte >> 4] + (strand - 1) * 5 + pass * 10
// of the nsite x 20 table (U+ACGTN, U-ACGTN, M+ACGTN, M-ACGTN).  The reference walks reads and sites as one merge
// (exact when both are sorted, its stated precondition); here a workgroup owns 256 consecutive rows:
//   1. the rows' smallest (rname, start) and largest (rname, end) bound ONE contiguous window of the sorted sites, found
//      by two 64-ary wavefront searches over the whole site list (ceil(log64 nsite) dependent loads each);
//   2. each row finds its sites inside the window (binary search in LDS when the window is staged there), a block scan
//      gives the (row, site) pairs a flat numbering, and the lanes stride over the pairs -- a 10 kb read or a deep
//      pile-up does not serialise one lane;
//   3. every pair is one byte load and one LDS counter increment; the window's nonzero counters go out with one global
//      atomicAdd each (neighbouring workgroups share their edge sites).  A window wider than BF_CAP sites (long reads,
//      dense site lists) counts with direct global atomics instead.
// Rows with a strand other than 1 / 2 (the placeholder template of an empty paired-end file has 0) are skipped.
#include <string.h>
#include "common.hpp"
#include "site_search.hpp"

namespace epi {

constexpr int BF_ROWS = 256;          // rows (= threads) per workgroup
constexpr int BF_CAP = 256;           // window sites counted in LDS: 20 u32 each
constexpr int BF_COLS = 20;

// site_key, wave_lower_bound, lds_lower_bound, glb_lower_bound and kNt16Int: site_search.hpp (shared with asm_report.hip)

__global__ __launch_bounds__(BF_ROWS) void k_base_freqs(const uint8_t *__restrict__ xm, const int64_t *__restrict__ off,
                                                        const int32_t *__restrict__ len, const int32_t *__restrict__ rname,
                                                        const int32_t *__restrict__ strand, const int32_t *__restrict__ start,
                                                        const int32_t *__restrict__ pass, int64_t n,
                                                        const int32_t *__restrict__ s_chr, const int32_t *__restrict__ s_pos,
                                                        int64_t nsite, uint32_t *__restrict__ counts) {
  __shared__ uint32_t cnt[BF_COLS * BF_CAP];        // [column][window site]
  __shared__ int64_t wkey[BF_CAP];
  __shared__ unsigned long long pre[BF_ROWS + 1], wsum[BF_ROWS / 64];   // pairs of the rows before row t; the scan's word per wave
  __shared__ int64_t r_base[BF_ROWS];               // off[x] - start[x]: the byte of position p is xm[r_base + p]
  __shared__ int32_t r_lo[BF_ROWS], r_col[BF_ROWS];
  __shared__ int64_t red_min[BF_ROWS / 64], red_max[BF_ROWS / 64];
  __shared__ int64_t win[2];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t x = (int64_t)blockIdx.x * BF_ROWS + t;
  int32_t rc = 0, st = 0, l = 0, sd = 0;
  if (x < n) { rc = rname[x]; st = start[x]; l = len[x]; sd = strand[x]; }
  const bool valid = x < n && (sd == 1 || sd == 2) && l > 0;
  const int64_t k_lo = valid ? site_key(rc, st) : INT64_MAX;
  const int64_t k_hi = valid ? site_key(rc, st) + l : INT64_MIN;     // key of (rname, end + 1)

  // 1. the window of sites the workgroup's rows can touch
  int64_t mn = k_lo, mx = k_hi;
  for (int d = 32; d >= 1; d >>= 1) {
    const int64_t a = __shfl_xor(mn, d, 64), c = __shfl_xor(mx, d, 64);
    mn = a < mn ? a : mn;
    mx = c > mx ? c : mx;
  }
  if (lane == 0) { red_min[wave] = mn; red_max[wave] = mx; }
  __syncthreads();
  mn = red_min[0]; mx = red_max[0];
  for (int w = 1; w < BF_ROWS / 64; w++) { mn = red_min[w] < mn ? red_min[w] : mn; mx = red_max[w] > mx ? red_max[w] : mx; }
  if (mx == INT64_MIN) return;                       // no countable row (uniform)
  if (wave < 2) {
    const int64_t r = wave_lower_bound(s_chr, s_pos, nsite, wave == 0 ? mn : mx);
    if (lane == 0) win[wave] = r;
  }
  __syncthreads();
  const int64_t lo = win[0], W = win[1] - win[0];
  if (W <= 0) return;
  const bool in_lds = W <= BF_CAP;
  if (in_lds) {
    for (int i = t; i < (int)W; i += BF_ROWS) wkey[i] = site_key(s_chr[lo + i], s_pos[lo + i]);
    for (int i = t; i < BF_COLS * BF_CAP; i += BF_ROWS) cnt[i] = 0;
    __syncthreads();
  }

  // 2. each row's sites inside the window, and the pairs numbered by a block scan
  int64_t c_row = 0;
  if (valid) {
    int64_t a, b;
    if (in_lds) { a = lds_lower_bound(wkey, (int32_t)W, k_lo); b = lds_lower_bound(wkey, (int32_t)W, k_hi); }
    else { a = glb_lower_bound(s_chr, s_pos, lo, lo + W, k_lo) - lo; b = glb_lower_bound(s_chr, s_pos, lo + a, lo + W, k_hi) - lo; }
    c_row = b - a;
    r_lo[t] = (int32_t)a;
    r_base[t] = off[x] - (int64_t)st;
    const int32_t p = pass ? pass[x] : 1;
    r_col[t] = (sd - 1) * 5 + (p != 0 ? 10 : 0);    // R logical: NA (INT_MIN) is TRUE
  }
  wg_scan_table<SumU64, BF_ROWS>((unsigned long long)c_row, pre, wsum);
  const uint64_t P = pre[BF_ROWS];

  // 3. one byte load and one counter per pair
  for (uint64_t j = t; j < P; j += BF_ROWS) {
    int32_t a = 0, b = BF_ROWS;                      // the row: last r with pre[r] <= j (it has pairs)
    while (b - a > 1) { const int32_t m = (a + b) >> 1; if (pre[m] <= j) a = m; else b = m; }
    const int32_t site = r_lo[a] + (int32_t)(j - pre[a]);
    const int32_t p = s_pos[lo + site];
    const uint32_t nib = xm[r_base[a] + p] >> 4;
    const int col = (int)((kNt16Int >> (4 * nib)) & 15u) + r_col[a];
    if (in_lds) atomicAdd(&cnt[col * BF_CAP + site], 1u);
    else atomicAdd(&counts[(int64_t)col * nsite + lo + site], 1u);
  }
  if (!in_lds) return;
  __syncthreads();
  for (int i = t; i < BF_COLS * (int)W; i += BF_ROWS) {
    const int col = i / (int)W, site = i - col * (int)W;
    const uint32_t c = cnt[col * BF_CAP + site];
    if (c) atomicAdd(&counts[(int64_t)col * nsite + lo + site], c);
  }
}

// sites must be sorted by (rname code, pos); equal keys (multi-ALT records) are allowed
__global__ __launch_bounds__(256) void k_sites_sorted(const int32_t *__restrict__ chr, const int32_t *__restrict__ pos, int64_t n,
                                                      uint32_t *__restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x + 1;
  const bool b = i < n && site_key(chr[i], pos[i]) < site_key(chr[i - 1], pos[i - 1]);
  if (__ballot(b) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}

}  // namespace epi

using namespace epi;

extern "C" int epi_batch_base_freqs_dev(epi_batch *b, const int32_t *d_pass, const int32_t *d_site_chr, const int32_t *d_site_pos,
                                        int64_t nsite, uint32_t *d_counts, void *stream) {
  if (!b || nsite < 0 || (nsite > 0 && (!d_site_chr || !d_site_pos || !d_counts)))
    return fail(EPI_ERR_ARG, "epi_batch_base_freqs_dev: bad arguments");
  if (nsite == 0) return EPI_OK;
  EPI_HIP(hipSetDevice(b->eng->device));
  hipStream_t s = pick_stream(b, stream);
  EPI_HIP(hipMemsetAsync(d_counts, 0, (size_t)nsite * BF_COLS * sizeof(uint32_t), s));
  EPI_TRY(b->bf_flag.ensure(sizeof(uint32_t)));
  uint32_t *d_bad = b->bf_flag.as<uint32_t>();
  EPI_HIP(hipMemsetAsync(d_bad, 0, sizeof(uint32_t), s));
  if (nsite > 1) {
    const int64_t nb = (nsite - 1 + 255) / 256;
    EPI_TRY(check_grid(nb, 256, "epi_batch_base_freqs_dev"));
    hipLaunchKernelGGL(k_sites_sorted, dim3((unsigned)nb), dim3(256), 0, s, d_site_chr, d_site_pos, nsite, d_bad);
    EPI_HIP(hipGetLastError());
  }
  uint32_t bad = 0;
  EPI_TRY(read_scalars(b, s, d_bad, sizeof(bad), &bad));
  if (bad) return fail(EPI_ERR_UNSORTED, "VCF sites are not sorted by (seqnames, start)");
  if (b->n == 0) return EPI_OK;
  EPI_TRY(fetch_row_stats(b, s));
  if (b->h_stats.bad_len) return fail(EPI_ERR_ARG, "offsets are not non-decreasing, or start+length exceeds int32");
  if (b->h_stats.unsorted)
    return fail(EPI_ERR_UNSORTED, "PRE-SORTED DATASET IS A REQUIREMENT: rows are not sorted by (rname, start)");
  const int64_t nb = (b->n + BF_ROWS - 1) / BF_ROWS;
  EPI_TRY(check_grid(nb, BF_ROWS, "epi_batch_base_freqs_dev"));
  prof_begin("base_freqs", s);
  hipLaunchKernelGGL(k_base_freqs, dim3((unsigned)nb), dim3(BF_ROWS), 0, s, b->xm, b->off, b->len, b->rname, b->strand, b->start,
                     d_pass, b->n, d_site_chr, d_site_pos, nsite, d_counts);
  EPI_HIP(hipGetLastError());
  prof_end("base_freqs", s);
  return EPI_OK;
}

// The drop-in form: host pointers, the caller's site order, a column-major nsite x 20 double matrix out.
extern "C" int epi_get_base_freqs(const uint8_t *xm, const int64_t *off, int64_t n, const int32_t *rname, const int32_t *strand,
                                  const int32_t *start, const int32_t *pass, const int32_t *site_chr, const int32_t *site_pos,
                                  int64_t nsite, double *out) {
  if (n < 0 || nsite < 0 || !off || (n > 0 && (!rname || !strand || !start)) ||
      (nsite > 0 && (!site_chr || !site_pos || !out)))
    return fail(EPI_ERR_ARG, "epi_get_base_freqs: bad arguments");
  if (nsite > 0) memset(out, 0, (size_t)nsite * BF_COLS * sizeof(double));
  // the non-NA sites, in the caller's order; they must be sorted (NA-coded ones match no read: zero rows)
  std::vector<int64_t> keep;
  std::vector<int32_t> kc, kp;
  for (int64_t i = 0; i < nsite; i++) {
    if (site_chr[i] == INT32_MIN) continue;
    if (!kc.empty() && (site_chr[i] < kc.back() || (site_chr[i] == kc.back() && site_pos[i] < kp.back())))
      return fail(EPI_ERR_UNSORTED, "VCF sites are not sorted by (seqnames, start)");
    keep.push_back(i); kc.push_back(site_chr[i]); kp.push_back(site_pos[i]);
  }
  epi_engine *eng;
  EPI_TRY(epi_default_engine(&eng));
  const int64_t m = (int64_t)keep.size();
  if (m == 0 || n == 0) return EPI_OK;
  epi_batch *b = nullptr;
  EPI_TRY(epi_batch_upload(eng, xm, off, rname, strand, start, n, &b));
  struct Guard {
    epi_batch *b; void *p[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Guard() { for (void *q : p) if (q) (void)hipFree(q); epi_batch_free(b); }
  } g{b};
  hipStream_t s = eng->stream;
  EPI_HIP(hipMalloc(&g.p[0], (size_t)m * 4));
  EPI_HIP(hipMalloc(&g.p[1], (size_t)m * 4));
  EPI_HIP(hipMalloc(&g.p[2], (size_t)m * BF_COLS * 4));
  EPI_HIP(hipMemcpyAsync(g.p[0], kc.data(), (size_t)m * 4, hipMemcpyHostToDevice, s));
  EPI_HIP(hipMemcpyAsync(g.p[1], kp.data(), (size_t)m * 4, hipMemcpyHostToDevice, s));
  if (pass) {
    EPI_HIP(hipMalloc(&g.p[3], (size_t)n * 4));
    EPI_HIP(hipMemcpyAsync(g.p[3], pass, (size_t)n * 4, hipMemcpyHostToDevice, s));
  }
  uint32_t *d_cnt = static_cast<uint32_t *>(g.p[2]);
  EPI_TRY(epi_batch_base_freqs_dev(b, static_cast<int32_t *>(g.p[3]), static_cast<int32_t *>(g.p[0]), static_cast<int32_t *>(g.p[1]),
                                   m, d_cnt, s));
  std::vector<uint32_t> h((size_t)m * BF_COLS);
  EPI_TRY(copy_to_host(eng, h.data(), d_cnt, h.size() * 4, s));
  for (int c = 0; c < BF_COLS; c++)
    for (int64_t k = 0; k < m; k++) out[(size_t)c * nsite + keep[k]] = (double)h[(size_t)c * m + k];
  return EPI_OK;
}
