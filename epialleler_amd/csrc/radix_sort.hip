// Stable LSD radix sort of (64-bit key, 32-bit value) pairs; radix_sort.hpp has the workspace (SortPairs) and its users.
// Least significant byte first, per byte the caller asks for: k_rsort_hist (a workgroup's tile of 4096 keys -> its column of
// the [digit][workgroup] table), util.hip's scan over the table, k_rsort_scatter.  The scatter is STABLE: a wave owns 1024
// consecutive keys of the tile and takes them 64 at a time; a key's rank among the wave's equal digits is the wave's running
// count of that digit (one lane per digit stores it, plain LDS stores) plus the number of lower lanes of the match mask
// (eight ballots).  No rank comes from what an LDS atomic returns.  The tile is put into digit order in LDS (keys, then
// values, in one 32 KB buffer) and stored from there, so that a wave's stores run along the digits' runs instead of 64 ways
// apart.
#include "radix_sort.hpp"

namespace epi {

// table[digit * nblk + workgroup] = keys of the workgroup's tile with that digit
__global__ __launch_bounds__(RSORT_WG) void k_rsort_hist(const uint64_t *__restrict__ key, uint32_t n, int shift, uint32_t nblk,
                                                         uint32_t *__restrict__ table) {
  __shared__ uint32_t s_hist[256];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)RSORT_TILE + (threadIdx.x >> 6) * (uint32_t)RSORT_WAVE_KEYS + (threadIdx.x & 63);
#pragma unroll
  for (int i = 0; i < RSORT_ITEMS; i++) {
    const uint32_t r = base + (uint32_t)i * 64u;
    const bool active = r < n;
    const uint32_t d = active ? (uint32_t)(key[r] >> shift) & 255u : 0u;
    hist_add(s_hist, d, active, __ballot(active));
  }
  __syncthreads();
  table[(size_t)threadIdx.x * nblk + blockIdx.x] = s_hist[threadIdx.x];
}

// off[digit * nblk + workgroup]: the exclusive scan of the table = where the workgroup's first key of that digit goes
__global__ __launch_bounds__(RSORT_WG) void k_rsort_scatter(const uint64_t *__restrict__ key_in, const uint32_t *__restrict__ row_in,
                                                            uint32_t n, int shift, uint32_t nblk, const uint32_t *__restrict__ off,
                                                            uint64_t *__restrict__ key_out, uint32_t *__restrict__ row_out) {
  __shared__ uint32_t s_cnt[RSORT_WAVES][256];      // per wave: keys of a digit seen so far; then: where in the tile its next key of the digit goes
  __shared__ uint64_t s_stage[RSORT_TILE];      // the tile's keys in digit order; then, as u32, its rows
  __shared__ uint32_t s_goff[256], s_wsum[RSORT_WAVES];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int w = 0; w < RSORT_WAVES; w++) s_cnt[w][threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)RSORT_TILE + wave * (uint32_t)RSORT_WAVE_KEYS + lane;
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t k[RSORT_ITEMS];
  uint32_t v[RSORT_ITEMS], rank[RSORT_ITEMS];
#pragma unroll
  for (int i = 0; i < RSORT_ITEMS; i++) {
    const uint32_t r = base + (uint32_t)i * 64u;
    const bool active = r < n;
    k[i] = active ? key_in[r] : 0ull;
    v[i] = active ? row_in[r] : 0u;
  }
#pragma unroll
  for (int i = 0; i < RSORT_ITEMS; i++) {
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
    uint32_t c[RSORT_WAVES], total = 0;
    for (int w = 0; w < RSORT_WAVES; w++) { c[w] = s_cnt[w][d]; total += c[w]; }
    const uint32_t start = wg_scan_excl<SumU32, RSORT_WG>(total, s_wsum);
    s_goff[d] = off[(size_t)d * nblk + blockIdx.x] - start;                   // (mod 2^32) + a key's place in the tile = its place in the output
    uint32_t at = start;
    for (int w = 0; w < RSORT_WAVES; w++) { s_cnt[w][d] = at; at += c[w]; }
  }
  __syncthreads();
  // the tile in digit order through LDS, so that a wave's stores run along the digits' runs: first the keys, then the rows
#pragma unroll
  for (int i = 0; i < RSORT_ITEMS; i++) {
    const bool active = base + (uint32_t)i * 64u < n;
    rank[i] += s_cnt[wave][(uint32_t)(k[i] >> shift) & 255u];                 // the key's place in the tile
    if (active && rank[i] < (uint32_t)RSORT_TILE) s_stage[rank[i]] = k[i];
  }
  __syncthreads();
  const uint32_t tile0 = blockIdx.x * (uint32_t)RSORT_TILE;
  const uint32_t count = n - tile0 < (uint32_t)RSORT_TILE ? n - tile0 : (uint32_t)RSORT_TILE;
  uint32_t dst[RSORT_ITEMS];
#pragma unroll
  for (int i = 0; i < RSORT_ITEMS; i++) {
    const uint32_t j = (uint32_t)i * RSORT_WG + threadIdx.x;
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
  for (int i = 0; i < RSORT_ITEMS; i++) {
    const bool active = base + (uint32_t)i * 64u < n;
    if (active && rank[i] < (uint32_t)RSORT_TILE) s_rows[rank[i]] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < RSORT_ITEMS; i++) {
    const uint32_t j = (uint32_t)i * RSORT_WG + threadIdx.x;
    if (j < count && dst[i] < n) row_out[dst[i]] = s_rows[j];
  }
}

int SortPairs::sort(uint32_t byte_mask, DevBuf &scan_tmp, hipStream_t s) {
  const int64_t nblk = radix_sort_blocks((int64_t)n);
  for (int d = 0; d < 8; d++) {
    if (!((byte_mask >> d) & 1u)) continue;
    prof_begin("rsort_hist", s);
    hipLaunchKernelGGL(k_rsort_hist, dim3((unsigned)nblk), dim3(RSORT_WG), 0, s, key[cur], n, 8 * d, (uint32_t)nblk, table[0]);
    prof_end("rsort_hist", s);
    prof_begin("rsort_table_scan", s);
    const int rc = scan_exclusive_u32(table[0], table[1], nblk * 256, nullptr, scan_tmp, s);
    prof_end("rsort_table_scan", s);
    EPI_TRY(rc);
    prof_begin("rsort_scatter", s);
    hipLaunchKernelGGL(k_rsort_scatter, dim3((unsigned)nblk), dim3(RSORT_WG), 0, s, key[cur], val[cur], n, 8 * d, (uint32_t)nblk,
                       table[1], key[cur ^ 1], val[cur ^ 1]);
    prof_end("rsort_scatter", s);
    cur ^= 1;
  }
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

}  // namespace epi
