// M-bias report: methylation by offset from either end of the template, per strand and context, and the totals per strand and
// context over every byte -- the table a user reads the `trim` of preprocessBam off, and the non-CpG totals that estimate the
// bisulfite conversion.  The reference has no such report; include/epihip.h, epi_batch_mbias_report_dev, has the interface.
//
// Definition (all integers).  Row x has strand s = strand[x] in {1, 2}, length L = len[x] and bytes b_0 .. b_{L-1} with codes
// c_i = b_i & 15.  A code has a class when it is one of 7 / 15 (CG methylated / unmethylated), 6 / 14 (CHG), 2 / 10 (CHH); every
// other code (5, 13, the filler 11, '.' 12, the unused ones) counts nowhere.  For every byte i with a class:
//   totals[s][ctx][state] += 1                                  (whatever max_offset is)
//   i < max_offset:          start[s][ctx][i][state] += 1
//   L - 1 - i < max_offset:  end[s][ctx][L - 1 - i][state] += 1
// A byte of a row shorter than 2 max_offset may count in both tables.  Offsets are template coordinates, filler included: the
// coordinates preprocessBam's trim cuts in.  No read rule, no thresholding; every row counts; rows need not be sorted.
//
// Data path, on the call's stream; nothing is kept on the batch:
//  (a) k_mbias: the TRANSPOSE of the per-read kernels' shape.  A workgroup walks a contiguous slice of rows and thread t owns
//      offset t (+ 256 j for max_offset > 256: NOFF offsets per thread) of both tables: per row, off / len / strand are
//      wave-uniform, thread t reads byte off + t and byte off + len - 1 - t (consecutive lanes, consecutive bytes; a thread
//      at or past len reads '.'), MB_RIF rows are loaded before any is counted.  The bytes of two rows and both ends form one
//      dword, one lut16_pick turns its four codes into four shift counts, and 1 << count is the code's one-hot in two words of
//      three 10-bit fields (methylated / unmethylated x CHH, CHG, CG; a code without a class shifts into bit 30, which no field
//      reads).  The words go to the accumulators of the row's strand (a uniform branch) and are flushed into 32-bit counters
//      every MB_FLUSH rows, before a field can carry.  No LDS, no atomics, no lane-varying register index.
//      The bytes no table owns (offsets >= max_offset from both ends, rows longer than 2 max_offset) feed the totals only: the
//      workgroup streams them as aligned 16-byte chunks, 256 threads x 16 bytes a step, through the same lookup.  A table byte's
//      total is the sum of the thread's own cells, less the bytes of short rows that both tables counted.
//  (b) every workgroup stores its cells (u32: a cell gets at most one count per row) and its twelve totals (u64) as partials;
//      k_mbias_reduce sums them into the caller's int64 arrays, 8 slices of the workgroups side by side.
// Integer sums: the result does not depend on the order of anything.
// EPI_MBIAS_LDS_ATOMIC (timing build, make timing-mbias): the shape this one replaced -- a wave per row, a lane per byte,
// LDS atomics into [end][strand][class][offset]; the rows of a workgroup hit the same bins of the same class.  Same results.
#include "common.hpp"

namespace epi {

constexpr int MB_WG = 256;              // threads of a workgroup = offsets a slot of the tables holds
constexpr int MB_RIF = 8;               // rows in flight: loaded before the first of them is counted
constexpr int MB_SLICE_MIN = 64;        // rows of a workgroup's slice, at least (a multiple of MB_RIF)
constexpr int MB_MAX_WG = 1024;         // workgroups of a call, at most (4 per CU)
constexpr int MB_FLUSH = 1016;          // rows between two flushes of the 10-bit fields: a multiple of MB_RIF, <= 1023
constexpr int MB_MID_FLUSH = 63;        // 16-byte chunks a thread counts between two flushes of the middle's fields: 1008 bytes
constexpr int MB_RED_SLICES = 8;        // the reduction's slices of the workgroups
constexpr int kMbiasMaxOffset = 1024;
constexpr uint32_t MB_NOCLASS = 30;     // the shift of a code without a class
// (every packed table field gets at most one count per row: W and DW are kept per offset slot)
static_assert(MB_FLUSH % MB_RIF == 0 && MB_FLUSH <= 1023 && MB_SLICE_MIN % MB_RIF == 0 && MB_MID_FLUSH * 16 <= 1023 && MB_RIF % 2 == 0, "M-bias geometry");

struct MbArgs {
  const uint8_t *xm;
  const int64_t *off;
  const int32_t *len, *strand;
  int64_t n, slice;                     // rows of the batch; rows per workgroup
  uint32_t M;                           // max_offset
  ClassLut F;                           // code -> shift count: 0 / 10 / 20 (methylated CHH, CHG, CG), 32 / 42 / 52 (unmethylated), else 30
  uint32_t *part;                       // [workgroups][24 M] cells, in the caller's order
  unsigned long long *ptot;             // [workgroups][12]
};

static ClassLut mbias_lut() {
  uint32_t f[16];
  for (int c = 0; c < 16; c++) f[c] = MB_NOCLASS;
  f[2] = 0; f[6] = 10; f[7] = 20; f[10] = 32; f[14] = 42; f[15] = 52;
  return lut16_pack(f);
}

// the one-hot words of the four codes of dword w: lo[l] / hi[l] = the methylated / unmethylated word of byte l
__device__ __forceinline__ void mb_dword(uint32_t w, const ClassLut &F, uint32_t (&lo)[4], uint32_t (&hi)[4]) {
  const uint32_t f = lut16_pick(w, F);
#pragma unroll
  for (int l = 0; l < 4; l++) {
    const unsigned long long one = 1ull << ((f >> (8 * l)) & 0xFFu);
    lo[l] = (uint32_t)one;
    hi[l] = (uint32_t)(one >> 32);
  }
}

// fields of a word pair into six counters [state * 3 + k]; sign -1 subtracts (u32 arithmetic wraps, the final sums do not)
__device__ __forceinline__ void mb_flush(uint32_t (&W)[2], uint32_t (&C)[6], bool subtract = false) {
#pragma unroll
  for (int st = 0; st < 2; st++)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const uint32_t v = (W[st] >> (10 * k)) & 0x3FFu;
      C[st * 3 + k] += subtract ? 0u - v : v;
    }
  W[0] = 0; W[1] = 0;
}

// bytes [lo, hi) of a dword kept, the others replaced by '.'
__device__ __forceinline__ uint32_t mb_keep_bytes(uint32_t w, int64_t lo, int64_t hi) {
  const int l = (int)(lo < 0 ? 0 : (lo > 4 ? 4 : lo));
  const int h = (int)(hi < 0 ? 0 : (hi > 4 ? 4 : hi));
  uint32_t m = 0u;
  if (h > l) m = (uint32_t)(((1ull << (8 * h)) - 1ull) & ~((1ull << (8 * l)) - 1ull));
  return (w & m) | (kXmDot4 & ~m);
}

#ifndef EPI_MBIAS_LDS_ATOMIC

template <int NOFF>
__global__ __launch_bounds__(MB_WG) void k_mbias(MbArgs a) {
  __shared__ unsigned long long s_tot[12];
  const uint32_t t = threadIdx.x, M = a.M;
  uint32_t W[NOFF][2][2][2];            // [slot][end][strand - 1][methylated, unmethylated]: three 10-bit fields each
  uint32_t C[NOFF][2][2][6];            // the cells: [state * 3 + k]
  uint32_t DW[NOFF][2][2];              // [slot][strand - 1]: the words of end bytes that the start table counted too -- per slot, as W:
                                        // a field then gets at most one count per row, whatever NOFF is
  uint32_t XW[2][2], T[2][6];           // the middle's words; T = the middle's counts less DW's
#pragma unroll
  for (int j = 0; j < NOFF; j++)
#pragma unroll
    for (int e = 0; e < 2; e++)
#pragma unroll
      for (int s = 0; s < 2; s++) {
        W[j][e][s][0] = 0; W[j][e][s][1] = 0;
        DW[j][s][0] = 0; DW[j][s][1] = 0;
#pragma unroll
        for (int c = 0; c < 6; c++) C[j][e][s][c] = 0;
      }
#pragma unroll
  for (int s = 0; s < 2; s++) {
    XW[s][0] = 0; XW[s][1] = 0;
#pragma unroll
    for (int c = 0; c < 6; c++) T[s][c] = 0;
  }
  if (t < 12) s_tot[t] = 0ull;
  __syncthreads();

  const auto flush_tables = [&]() {
#pragma unroll
    for (int j = 0; j < NOFF; j++)
#pragma unroll
      for (int e = 0; e < 2; e++)
#pragma unroll
        for (int s = 0; s < 2; s++) mb_flush(W[j][e][s], C[j][e][s]);
#pragma unroll
    for (int j = 0; j < NOFF; j++)
#pragma unroll
      for (int s = 0; s < 2; s++) mb_flush(DW[j][s], T[s], true);
  };
  const auto flush_middle = [&]() {
#pragma unroll
    for (int s = 0; s < 2; s++) mb_flush(XW[s], T[s]);
  };

  const int64_t r0 = (int64_t)blockIdx.x * a.slice;
  const int64_t r1 = r0 + a.slice < a.n ? r0 + a.slice : a.n;
  uint32_t since = 0, mid_pending = 0;  // rows since the tables' flush; chunks a thread may hold since the middle's
  for (int64_t rb = r0; rb < r1; rb += MB_RIF) {
    int64_t o[MB_RIF];
    uint32_t L[MB_RIF];
    bool rev[MB_RIF];
#pragma unroll
    for (int q = 0; q < MB_RIF; q++) {  // wave-uniform: the row's offset, length and strand
      const int64_t row = rb + q < r1 ? rb + q : r1 - 1;
      o[q] = a.off[row];
      L[q] = rb + q < r1 ? (uint32_t)a.len[row] : 0u;
      rev[q] = __builtin_amdgcn_readfirstlane(a.strand[row]) == 2;
    }
    // the tables: byte d from either end
#pragma unroll
    for (int j = 0; j < NOFF; j++) {
      if ((uint32_t)(j * MB_WG) + (t & ~63u) >= M) break;     // (per wave: none of its lanes owns an offset of this slot)
      const uint32_t d = t + (uint32_t)(j * MB_WG);
      const bool own = d < M;
      uint32_t by[MB_RIF][2];
#pragma unroll
      for (int q = 0; q < MB_RIF; q++) {
        const bool valid = own && d < L[q];
        const uint8_t *p = a.xm + o[q];
        by[q][0] = valid ? (uint32_t)p[d] : kXmDot;
        by[q][1] = valid ? (uint32_t)p[L[q] - 1u - d] : kXmDot;
      }
#pragma unroll
      for (int q2 = 0; q2 < MB_RIF; q2 += 2) {
        const uint32_t w = by[q2][0] | (by[q2][1] << 8) | (by[q2 + 1][0] << 16) | (by[q2 + 1][1] << 24);
        uint32_t lo[4], hi[4];
        mb_dword(w, a.F, lo, hi);
#pragma unroll
        for (int l = 0; l < 4; l++) {
          const int q = q2 + (l >> 1), e = l & 1;
          if (rev[q]) { W[j][e][1][0] += lo[l]; W[j][e][1][1] += hi[l]; }
          else { W[j][e][0][0] += lo[l]; W[j][e][0][1] += hi[l]; }
          if (e == 1 && L[q] < 2u * M) {            // a short row: its end byte at L - 1 - d < M is in the start table too
            const bool dup = L[q] - 1u - d < M;     // (a thread at or past L holds '.': bit 30 and nothing else)
            const uint32_t dlo = dup ? lo[l] : 0u, dhi = dup ? hi[l] : 0u;
            if (rev[q]) { DW[j][1][0] += dlo; DW[j][1][1] += dhi; }
            else { DW[j][0][0] += dlo; DW[j][0][1] += dhi; }
          }
        }
      }
    }
    since += MB_RIF;
    if (since >= (uint32_t)MB_FLUSH) { flush_tables(); since = 0; }
    // the middle: bytes [M, L - M) of rows longer than 2 M, for the totals alone
    // (a loop that is not unrolled: it reads the row's scalars again instead of indexing the registers above)
#pragma unroll 1
    for (int64_t row = rb; row < r1 && row < rb + MB_RIF; row++) {
      const uint32_t Lq = (uint32_t)a.len[row];
      if (Lq <= 2u * M) continue;
      const int64_t oq = a.off[row];
      const bool revq = __builtin_amdgcn_readfirstlane(a.strand[row]) == 2;
      const int64_t b0 = oq + (int64_t)M, b1 = oq + (int64_t)Lq - (int64_t)M;
      const int64_t c1 = (b1 + 15) >> 4;
      const auto stream = [&](uint32_t (&X)[2]) {
        for (int64_t cb = b0 >> 4; cb < c1; cb += MB_WG) {
          if (mid_pending == (uint32_t)MB_MID_FLUSH) { flush_middle(); mid_pending = 0; }
          mid_pending++;
          const int64_t c = cb + t;
          if (c >= c1) continue;
          const int64_t g0 = c << 4;
          uint4 v = *reinterpret_cast<const uint4 *>(a.xm + g0);
          if (g0 < b0 || g0 + 16 > b1) {            // the first and the last chunk: foreign bytes read as '.'
            v.x = mb_keep_bytes(v.x, b0 - g0, b1 - g0);
            v.y = mb_keep_bytes(v.y, b0 - g0 - 4, b1 - g0 - 4);
            v.z = mb_keep_bytes(v.z, b0 - g0 - 8, b1 - g0 - 8);
            v.w = mb_keep_bytes(v.w, b0 - g0 - 12, b1 - g0 - 12);
          }
          const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int u = 0; u < 4; u++) {
            uint32_t lo[4], hi[4];
            mb_dword(vw[u], a.F, lo, hi);
            X[0] += (lo[0] + lo[1]) + (lo[2] + lo[3]);
            X[1] += (hi[0] + hi[1]) + (hi[2] + hi[3]);
          }
        }
      };
      if (revq) stream(XW[1]); else stream(XW[0]);
    }
  }
  flush_tables();
  flush_middle();

  // the workgroup's partials: every cell of its threads, zeros included (the partials are not cleared)
  uint32_t *part = a.part + (size_t)blockIdx.x * 24u * M;
  uint32_t tot[2][6];
#pragma unroll
  for (int s = 0; s < 2; s++)
#pragma unroll
    for (int c = 0; c < 6; c++) tot[s][c] = T[s][c];
#pragma unroll
  for (int j = 0; j < NOFF; j++) {
    const uint32_t d = t + (uint32_t)(j * MB_WG);
#pragma unroll
    for (int e = 0; e < 2; e++)
#pragma unroll
      for (int s = 0; s < 2; s++)
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
          for (int st = 0; st < 2; st++) {
            const uint32_t v = C[j][e][s][st * 3 + k];
            tot[s][st * 3 + k] += v;                // (a thread past M holds zeros)
            if (d < M) part[((((uint32_t)(e * 2 + s) * 3u + k) * M + d) * 2u) + st] = v;
          }
  }
  // twelve totals over the workgroup: halves of 16 bits summed over the wave, 64-bit adds in LDS
#pragma unroll
  for (int s = 0; s < 2; s++)
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int st = 0; st < 2; st++) {
        const uint32_t v = tot[s][st * 3 + k];
        const unsigned long long sum = (unsigned long long)wave_sum_u32(v & 0xFFFFu) + ((unsigned long long)wave_sum_u32(v >> 16) << 16);
        if ((t & 63u) == 0u && sum) atomicAdd(&s_tot[(s * 3 + k) * 2 + st], sum);
      }
  __syncthreads();
  if (t < 12) a.ptot[(size_t)blockIdx.x * 12u + t] = s_tot[t];
}

#else  // EPI_MBIAS_LDS_ATOMIC: a wave per row, a lane per byte, LDS atomics into the bins (timing build)

template <int NOFF>
__global__ __launch_bounds__(MB_WG) void k_mbias(MbArgs a) {
  extern __shared__ uint32_t s_bin[];   // [24 M] in the caller's order
  __shared__ unsigned long long s_tot[12];
  const uint32_t t = threadIdx.x, M = a.M, lane = t & 63u;
  for (uint32_t i = t; i < 24u * M; i += MB_WG) s_bin[i] = 0u;
  if (t < 12) s_tot[t] = 0ull;
  __syncthreads();
  uint32_t X[2][2] = {{0, 0}, {0, 0}}, T[2][6];
#pragma unroll
  for (int s = 0; s < 2; s++)
#pragma unroll
    for (int c = 0; c < 6; c++) T[s][c] = 0;
  uint32_t pending = 0;
  const int64_t r0 = (int64_t)blockIdx.x * a.slice;
  const int64_t r1 = r0 + a.slice < a.n ? r0 + a.slice : a.n;
  for (int64_t row = r0 + (t >> 6); row < r1; row += MB_WG / 64) {
    const int64_t o = a.off[row];
    const uint32_t L = (uint32_t)a.len[row];
    const uint32_t s = __builtin_amdgcn_readfirstlane(a.strand[row]) == 2 ? 1u : 0u;
    for (uint32_t i0 = 0; i0 < L; i0 += 64u) {
      if (pending == 1023u) { mb_flush(X[0], T[0]); mb_flush(X[1], T[1]); pending = 0; }
      pending++;
      const uint32_t i = i0 + lane;
      if (i >= L) continue;
      const uint32_t f = lut16_pick((uint32_t)a.xm[o + i], a.F) & 0xFFu;
      if (f == MB_NOCLASS) continue;
      const unsigned long long one = 1ull << f;
      if (s) { X[1][0] += (uint32_t)one; X[1][1] += (uint32_t)(one >> 32); } else { X[0][0] += (uint32_t)one; X[0][1] += (uint32_t)(one >> 32); }
      const uint32_t st = f >= 32u ? 1u : 0u, k = (f & 31u) / 10u;
      if (i < M) atomicAdd(&s_bin[(((0u * 2u + s) * 3u + k) * M + i) * 2u + st], 1u);
      if (L - 1u - i < M) atomicAdd(&s_bin[(((1u * 2u + s) * 3u + k) * M + (L - 1u - i)) * 2u + st], 1u);
    }
  }
  mb_flush(X[0], T[0]); mb_flush(X[1], T[1]);
  __syncthreads();
  uint32_t *part = a.part + (size_t)blockIdx.x * 24u * M;
  for (uint32_t i = t; i < 24u * M; i += MB_WG) part[i] = s_bin[i];
#pragma unroll
  for (int s = 0; s < 2; s++)
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
      for (int st = 0; st < 2; st++) {
        const uint32_t v = T[s][st * 3 + k];
        const unsigned long long sum = (unsigned long long)wave_sum_u32(v & 0xFFFFu) + ((unsigned long long)wave_sum_u32(v >> 16) << 16);
        if (lane == 0u && sum) atomicAdd(&s_tot[(s * 3 + k) * 2 + st], sum);
      }
  __syncthreads();
  if (t < 12) a.ptot[(size_t)blockIdx.x * 12u + t] = s_tot[t];
}

#endif

// counts[i] += the cell's partials of this slice of the workgroups (counts and totals zeroed in front of the kernel)
__global__ __launch_bounds__(256) void k_mbias_reduce(const uint32_t *__restrict__ part, const unsigned long long *__restrict__ ptot, uint32_t nwg,
                                                      uint32_t ncell, unsigned long long *__restrict__ counts, unsigned long long *__restrict__ totals) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t per = (nwg + gridDim.y - 1u) / gridDim.y;
  const uint32_t g0 = blockIdx.y * per, g1 = g0 + per < nwg ? g0 + per : nwg;
  if (i < ncell) {
    unsigned long long sum = 0;
    for (uint32_t g = g0; g < g1; g++) sum += part[(size_t)g * ncell + i];
    if (sum) atomicAdd(&counts[i], sum);
  }
  if (blockIdx.x == 0 && threadIdx.x < 12u) {
    unsigned long long sum = 0;
    for (uint32_t g = g0; g < g1; g++) sum += ptot[(size_t)g * 12u + threadIdx.x];
    if (sum) atomicAdd(&totals[threadIdx.x], sum);
  }
}

// both kernels behind each other on the stream (the caller drains it on every return path)
static int mbias_launch(const MbArgs &a, int64_t nwg, uint32_t ncell, int64_t *d_counts, int64_t *d_totals, hipStream_t s) {
  prof_begin("mbias_report", s);
#ifdef EPI_MBIAS_LDS_ATOMIC
  const size_t lds = (size_t)ncell * 4;
  if (lds > 64 * 1024) EPI_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mbias<1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_mbias<1>), dim3((unsigned)nwg), dim3(MB_WG), lds, s, a);
#else
  switch ((a.M + MB_WG - 1) / MB_WG) {
    case 1: hipLaunchKernelGGL((k_mbias<1>), dim3((unsigned)nwg), dim3(MB_WG), 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_mbias<2>), dim3((unsigned)nwg), dim3(MB_WG), 0, s, a); break;
    case 3: hipLaunchKernelGGL((k_mbias<3>), dim3((unsigned)nwg), dim3(MB_WG), 0, s, a); break;
    default: hipLaunchKernelGGL((k_mbias<4>), dim3((unsigned)nwg), dim3(MB_WG), 0, s, a); break;
  }
#endif
  EPI_HIP(hipGetLastError());
  const unsigned ry = (unsigned)(nwg < MB_RED_SLICES ? nwg : MB_RED_SLICES);
  hipLaunchKernelGGL(k_mbias_reduce, dim3((ncell + 255u) / 256u, ry), dim3(256), 0, s, a.part, a.ptot, (uint32_t)nwg, ncell,
                     reinterpret_cast<unsigned long long *>(d_counts), reinterpret_cast<unsigned long long *>(d_totals));
  EPI_HIP(hipGetLastError());
  prof_end("mbias_report", s);
  return EPI_OK;
}

static int mbias_report(epi_batch *b, int32_t max_offset, int64_t *d_counts, int64_t *d_totals, hipStream_t s) {
  const char *who = "epi_batch_mbias_report_dev";
  const uint32_t M = (uint32_t)max_offset, ncell = 24u * M;
  if (b->n > 0) {
    EPI_TRY(fetch_row_stats(b, s));
    if (b->h_stats.bad_len) return fail(EPI_ERR_ARG, "offsets are not non-decreasing, or start+length exceeds int32");
    if (b->h_stats.bad_strand) return fail(EPI_ERR_ARG, "strand values must be 1 ('+') or 2 ('-')");
  }
  EPI_HIP(hipMemsetAsync(d_counts, 0, (size_t)ncell * 8, s));
  EPI_HIP(hipMemsetAsync(d_totals, 0, 12 * 8, s));
  if (b->n == 0) return EPI_OK;
  // the slices: MB_SLICE_MIN rows at least, MB_MAX_WG workgroups at the most (a slice stays under 2^31 rows: u32 cells)
  int64_t nwg = (b->n + MB_SLICE_MIN - 1) / MB_SLICE_MIN;
  if (nwg > MB_MAX_WG) nwg = MB_MAX_WG;
  if (b->n / nwg >= (1LL << 31)) nwg = b->n >> 30;
  int64_t slice = (b->n + nwg - 1) / nwg;
  slice = (slice + MB_RIF - 1) / MB_RIF * MB_RIF;
  EPI_TRY(check_grid(nwg, MB_WG, who));
  DevBuf d_part, d_ptot;                                      // the call's scratch: goes with it on every return path
  EPI_TRY(d_part.ensure((size_t)nwg * ncell * 4));
  EPI_TRY(d_ptot.ensure((size_t)nwg * 12 * 8));
  MbArgs a;
  a.xm = b->xm; a.off = b->off; a.len = b->len; a.strand = b->strand;
  a.n = b->n; a.slice = slice; a.M = M; a.F = mbias_lut();
  a.part = d_part.as<uint32_t>(); a.ptot = d_ptot.as<unsigned long long>();
  // whatever the launches return, the stream is drained before the scratch goes: a kernel may already be running on it
  const int rc = mbias_launch(a, nwg, ncell, d_counts, d_totals, s);
  const hipError_t drained = hipStreamSynchronize(s);
  EPI_TRY(rc);
  EPI_HIP(drained);
  return EPI_OK;
}

}  // namespace epi

using namespace epi;

extern "C" {

int epi_batch_mbias_report_dev(epi_batch *b, int32_t max_offset, int64_t *d_counts, int64_t *d_totals, void *stream) {
  const char *who = "epi_batch_mbias_report_dev";
  if (!b) return fail(EPI_ERR_ARG, "%s: batch is NULL", who);
  if (max_offset < 1 || max_offset > kMbiasMaxOffset) return fail(EPI_ERR_ARG, "%s: max_offset = %d, 1 to %d offsets", who, max_offset, kMbiasMaxOffset);
  if (!d_counts) return fail(EPI_ERR_ARG, "%s: d_counts is NULL", who);
  if (!d_totals) return fail(EPI_ERR_ARG, "%s: d_totals is NULL", who);
  EPI_HIP(hipSetDevice(b->eng->device));
  return mbias_report(b, max_offset, d_counts, d_totals, pick_stream(b, stream));
}

}  // extern "C"
