// Region report: read-level statistics of the calls that the kept rows have inside every region of a list -- the methylated
// haplotype load of Guo et al. 2017 (mhl), and what the mHap tool-chain reports per interval: mean methylation (beta), the
// share of discordant reads (pdr), of reads with a methylated call (chalm), the cytosines unmethylated on such reads (mcr), the
// methylation block score (mbs) and the U / X / M read fractions.  No reference interface is replaced; include/epihip.h,
// epi_batch_region_report_dev, has the interface.
//
// Definitions.  ctx: context letters in both cases; max_oo = max_ooctx_meth_frac.
//  Kept rows   row x is kept by the lMHL read rule with hmin = 0 over the whole row (rcpp_mhl_report.cpp:172-179; the verdict of
//              xm_codes.hpp): o_m / (o_m + o_u) > max_oo drops it, o_m / o_u = its methylated (codes 2, 5, 6, 7) /
//              unmethylated (10, 13, 14, 15) bytes whose code is not one of ctx's; 0 / 0 is NaN and keeps the row.
//  Calls       of a kept row in region [start, end] on its rname: its bytes whose context code is one of ctx's letters and
//              whose position start[x] + i - (strand == 2 ? reverse_offset : 0) lies in [start, end], in row order.
//              n = their number, m = the methylated ones, r_1 .. r_q = the lengths of the maximal runs of methylated calls.
//              The row is COUNTED when 1 <= n <= max_sites and a K-READ when also n >= min_sites.
//  Integers    nreads: rows with n >= 1.  nlong: rows with n > max_sites (in nreads and nowhere else).  maxsites: the largest
//              n of a counted row.  Over counted rows: tbase = sum n, mbase = sum m, cbase = sum (n - m) over rows with
//              m >= 1.  Over k-reads: kreads their number, ndiscordant those with 0 < m < n, nmethylated those with m >= 1,
//              n_u those with (double)m <= u_max * (double)n, n_m those of the rest with (double)m >= m_min * (double)n,
//              n_x what remains.
//  Per length  l = 1 .. max_sites: H[n] = counted rows with n sites; M[l] = sum over counted rows and their runs of
//              max(0, r_j - l + 1); S2[n] = sum over k-reads with n sites of sum_j r_j^2.  The device keeps R[r], the number
//              of runs of length r of counted rows, in place of M: M[l] = sum_{r >= l} R[r] (r - l + 1).  All integers: every
//              accumulation is an integer add and no result depends on the order of arrival.
//  Ratios      fp64, each evaluated once per region by one thread, in this order; a zero denominator gives NaN.
//              beta = mbase / tbase, pdr = ndiscordant / kreads, chalm = nmethylated / kreads, mcr = cbase / tbase,
//              mbs = (sum_{n = min_sites}^{maxsites} S2[n] / (n n)) / kreads in ascending n,
//              mhl = (sum_{l = 1}^{maxsites} l (M[l] / T[l])) / (sum_{l = 1}^{maxsites} l) in ascending l,
//              T[l] = sum_n H[n] max(0, n - l + 1) (positive for every l <= maxsites).
//
// Data path, all on the call's stream; nothing is kept on the batch:
//  (a) k_rgn_ranges: rows sorted by (rname, start), one thread per region finds its candidate rows by search (pat_search.hpp,
//      shared with the pattern calls): those of its rname that start in [start - Lmax + 1, end + reverse_offset].  The
//      ranges come to the host (the call's first synchronisation).
//  (b) Consecutive regions form a GROUP while their counters ((3 max_sites + 16) u64 each) and bookkeeping stay under the cap
//      (256 MiB; EPIHIP_RGN_GROUP_BYTES; a region above it runs alone).  The ranges of a group laid end to end are one flat list
//      of (region, row) pairs under a u64 scan, pre[].
//  (c) k_rgn_count: a workgroup takes a chunk of consecutive pairs, a group of G lanes (16, or 64 for long rows) a pair.  The
//      group walks its row ONCE, four bytes per lane and step: the read rule's two counts over the whole row, and in the
//      steps that touch the region's span the calls, as eight ballots (byte j of every lane: a call, methylated) that every
//      lane of the group reads in row order -- n, m, the sum of r^2 and the run lengths (parked in LDS until the row's n is
//      known: at most 128 runs while n <= 256).
//      Accumulation: the pairs of a region are contiguous, so a chunk is a sequence of SEGMENTS of one region each.  The
//      workgroup counts a segment in LDS (u32: a chunk holds 512 pairs at most) and adds the non-zero counters to the
//      region's u64 counters in global memory once per segment.  A chunk is 1 to 32 rounds of the workgroup's 16 (or 4)
//      groups: as few as spread the call over 2048 workgroups, so that shallow regions run side by side, 32 for deep ones.  An amplicon of 10^6 rows gets ~2000 workgroups x ~30 adds
//      instead of 10^7 adds to a few dozen addresses (the cliff of profiles/summarise_patterns.txt); 10^5 shallow regions
//      get one add per region and non-zero counter.  EPI_RGN_PER_ROW (timing build): every row adds to global memory.
//  (d) k_rgn_finish: a thread per region evaluates the ratios in the order above and writes the 21 columns; a count that
//      does not fit int32 is reported, not wrapped.  The call's second synchronisation reads that verdict.
#include "common.hpp"
#include "pat_search.hpp"
#include "site_table.hpp"
#include <math.h>
#include <vector>

namespace epi {

constexpr int RGN_WG = 256;
constexpr int RGN_ROUNDS = 32;                     // pairs per group and chunk, at the most
constexpr int64_t RGN_BLOCKS = 2048;               // workgroups a call is spread over before its chunks grow
constexpr int kRgnMaxSites = 256;
constexpr int RGN_HDR = 16;                        // scalar counters in front of H, R and S2
constexpr int RGN_MAXRUNS = kRgnMaxSites / 2;      // runs of a row with n <= 256: every run but the last is followed by a call
constexpr int64_t kRgnGroupBytes = 256LL << 20;
enum { RC_NREADS = 0, RC_NLONG, RC_KREADS, RC_TBASE, RC_MBASE, RC_CBASE, RC_NDISC, RC_NMETH, RC_NU, RC_NX, RC_NM };

struct RgnTarget {                // a region of a group, as a segment's workgroup reads it
  int64_t row_lo;                 // its candidate rows: row_lo + (j - pre[t])
  int32_t start, end;
};

struct RgnArgs {
  const uint8_t *xm;
  const int64_t *off;
  const int32_t *len, *strand, *start;
  const uint64_t *pre;            // [ng + 1]
  const int64_t *row_lo;          // [ng] first candidate row
  const int32_t *rs, *re;         // [ng] the group's regions in the caller's arrays
  unsigned long long *cnt;        // [ng][stride]
  uint64_t npairs;
  int32_t ng;
  uint32_t rounds;                // pairs per group and chunk: 1 .. RGN_ROUNDS
  uint32_t stride;                // RGN_HDR + 3 * max_sites
  uint32_t ctx_mask, oom_mask, oou_mask;
  int32_t min_sites, max_sites, reverse_offset;
  double u_max, m_min, max_oo;
};

__global__ __launch_bounds__(256) void k_rgn_ranges(const int32_t *__restrict__ rname, const int32_t *__restrict__ start, int64_t n,
                                                    const int32_t *__restrict__ chr, const int32_t *__restrict__ rs, const int32_t *__restrict__ re,
                                                    int32_t nt, int64_t lmax, int64_t reverse_offset, int64_t *__restrict__ rng) {
  const int32_t t = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (t >= nt) return;
  const int32_t qr = chr[t];
  const int64_t lo = pat_row_lower_bound(rname, start, n, qr, (int64_t)rs[t] - lmax + 1);
  int64_t hi = pat_row_lower_bound(rname, start, n, qr, (int64_t)re[t] + reverse_offset + 1);
  if (hi < lo) hi = lo;
  rng[2 * (int64_t)t] = lo;
  rng[2 * (int64_t)t + 1] = hi;
}

// One pair: the G lanes of a group walk row x once and lane 0 of the group adds what the row gives its region through
// add(counter, value).  Every lane of the wave calls this together (have: the group has a pair); runs: RGN_MAXRUNS entries of
// the group's own.
template <int G, class Add>
__device__ __forceinline__ void rgn_row(const RgnArgs &a, const RgnTarget &tg, int64_t x, bool have, uint32_t sub, uint32_t grp,
                                        uint16_t *runs, Add add) {
  const int32_t len = have ? a.len[x] : 0;
  const uint8_t *p = a.xm + (have ? a.off[x] : 0);
  const int64_t shift = have ? (int64_t)a.start[x] - (a.strand[x] == 2 ? (int64_t)a.reverse_offset : 0) : 0;   // byte i is at shift + i
  int64_t i0 = (int64_t)tg.start - shift, i1 = (int64_t)tg.end - shift + 1;                                     // the region's bytes: [i0, i1)
  if (i0 < 0) i0 = 0;
  if (i1 > len) i1 = len;
  uint32_t om = 0, ou = 0, n = 0, m = 0, run = 0, q = 0, s2 = 0;
  const auto close_run = [&]() {
    s2 += run * run;
    if (sub == 0 && q < (uint32_t)RGN_MAXRUNS) runs[q] = (uint16_t)run;
    q++;
    run = 0;
  };
  const uint32_t ulen = (uint32_t)len;                         // (unsigned: the step behind a row of 2^31 - 1 bytes does not wrap)
  for (uint32_t c = 0; __ballot(c < ulen) != 0ull; c += 4u * G) {
    const uint32_t my = c + 4u * sub;
    uint32_t w = kXmDot4;                                      // '.': in no class, no call
    if (my + 4u <= ulen) memcpy(&w, p + my, 4);
    else for (uint32_t j = 0; my + j < ulen; j++) w = (w & ~(0xFFu << (8 * j))) | ((uint32_t)p[my + j] << (8 * j));
    uint32_t vb = 0, mb = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t nib = (w >> (8 * j)) & 15u;
      om += (a.oom_mask >> nib) & 1u;
      ou += (a.oou_mask >> nib) & 1u;
      const int64_t i = (int64_t)my + j;
      const bool call = ((a.ctx_mask >> nib) & 1u) != 0u && i >= i0 && i < i1;
      vb |= (call ? 1u : 0u) << j;
      mb |= (call && nib < 8u ? 1u : 0u) << j;
    }
    unsigned long long V[4], M[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      V[j] = group_ballot<G>((int)((vb >> j) & 1u), grp);
      M[j] = group_ballot<G>((int)((mb >> j) & 1u), grp);
    }
    unsigned long long any = V[0] | V[1] | V[2] | V[3];       // the group's lanes that hold a call, in row order
    while (any) {
      const int l = __ffsll((long long)any) - 1;
      any &= any - 1ull;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (!((V[j] >> l) & 1ull)) continue;
        n++;
        if ((M[j] >> l) & 1ull) { m++; run++; }
        else if (run) close_run();
      }
    }
  }
  if (run) close_run();
#pragma unroll
  for (int d = 1; d < G; d <<= 1) { om += __shfl_xor(om, d, 64); ou += __shfl_xor(ou, d, 64); }
  if (!have || sub != 0 || !read_rule_keeps(1, om, ou, a.max_oo) || n == 0) return;   // (an empty row has n == 0)
  const uint32_t ms = (uint32_t)a.max_sites;
  add(RC_NREADS, 1u);
  if (n > ms) { add(RC_NLONG, 1u); return; }
  add(RC_TBASE, n);
  if (m) { add(RC_MBASE, m); if (n > m) add(RC_CBASE, n - m); }
  add(RGN_HDR + (n - 1u), 1u);                                          // H[n]
  for (uint32_t j = 0; j < q && j < (uint32_t)RGN_MAXRUNS; j++) add(RGN_HDR + ms + ((uint32_t)runs[j] - 1u), 1u);   // R[r]
  if (n < (uint32_t)a.min_sites) return;
  add(RC_KREADS, 1u);
  if (m > 0 && m < n) add(RC_NDISC, 1u);
  if (m) add(RC_NMETH, 1u);
  if ((double)m <= a.u_max * (double)n) add(RC_NU, 1u);
  else if ((double)m >= a.m_min * (double)n) add(RC_NM, 1u);
  else add(RC_NX, 1u);
  if (s2) add(RGN_HDR + 2u * ms + (n - 1u), s2);                        // S2[n]
}

template <int G>
__global__ __launch_bounds__(RGN_WG) void k_rgn_count(RgnArgs a) {
  constexpr int NGRP = RGN_WG / G;
  const uint64_t CHUNK = (uint64_t)NGRP * a.rounds;
#ifndef EPI_RGN_PER_ROW
  __shared__ uint32_t s_cnt[RGN_HDR + 3 * kRgnMaxSites];
#endif
  __shared__ uint16_t s_run[NGRP][RGN_MAXRUNS];
  const uint32_t lane = threadIdx.x & 63u, sub = lane % G, grp = lane / G, g = threadIdx.x / G;
  const uint64_t c0 = (uint64_t)blockIdx.x * CHUNK;
  const uint64_t c1 = c0 + CHUNK < a.npairs ? c0 + CHUNK : a.npairs;
  for (uint64_t j = c0; j < c1;) {                            // a segment: the chunk's pairs of one region
    const int32_t t = pat_target_of(a.pre, a.ng, j);
    const uint64_t p0 = a.pre[t], p1 = a.pre[t + 1];
    const uint64_t seg_end = p1 < c1 ? p1 : c1;
    RgnTarget tg;
    tg.row_lo = a.row_lo[t]; tg.start = a.rs[t]; tg.end = a.re[t];
    unsigned long long *gc = a.cnt + (size_t)t * a.stride;
#ifdef EPI_RGN_PER_ROW
    const auto add = [&](uint32_t i, uint32_t v) { atomicAdd(gc + i, (unsigned long long)v); };
#else
    for (uint32_t i = threadIdx.x; i < a.stride; i += RGN_WG) s_cnt[i] = 0u;
    __syncthreads();
    const auto add = [&](uint32_t i, uint32_t v) { atomicAdd(&s_cnt[i], v); };
#endif
    for (uint64_t pb = j; pb < seg_end; pb += NGRP) {
      const uint64_t pr = pb + g;
      const bool have = pr < seg_end;
      rgn_row<G>(a, tg, tg.row_lo + (int64_t)(pr - p0), have, sub, grp, s_run[g], add);
    }
#ifndef EPI_RGN_PER_ROW
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < a.stride; i += RGN_WG) {
      const uint32_t v = s_cnt[i];
      if (v) atomicAdd(gc + i, (unsigned long long)v);
    }
    __syncthreads();
#endif
    j = seg_end;
  }
}

struct RgnOut {
  int32_t *icol[15];              // rname, start, end, nreads, nlong, kreads, tbase, mbase, cbase, ndiscordant, nmethylated, n_u, n_x, n_m, maxsites
  double *dcol[6];                // beta, pdr, chalm, mcr, mbs, mhl
};

__device__ __forceinline__ double rgn_ratio(unsigned long long a, unsigned long long b) {
  return b ? (double)a / (double)b : (double)NAN;
}

// regions [t0, t0 + ng) of the call, counters cnt[ng][stride]; *bad = 1 + the last region with a count above int32
__global__ __launch_bounds__(256) void k_rgn_finish(const unsigned long long *__restrict__ cnt, uint32_t stride, int32_t ng, int32_t t0,
                                                    const int32_t *__restrict__ chr, const int32_t *__restrict__ rs, const int32_t *__restrict__ re,
                                                    int32_t min_sites, int32_t max_sites, RgnOut o, uint32_t *__restrict__ bad) {
  const int32_t k = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (k >= ng) return;
  const unsigned long long *c = cnt + (size_t)k * stride;
  const unsigned long long *H = c + RGN_HDR - 1, *R = H + max_sites, *S2 = R + max_sites;     // indexed 1 .. max_sites
  const int32_t t = t0 + k;
  int32_t maxsites = max_sites;
  while (maxsites > 0 && H[maxsites] == 0ull) maxsites--;
  const unsigned long long nreads = c[RC_NREADS], nlong = c[RC_NLONG], kreads = c[RC_KREADS], tbase = c[RC_TBASE], mbase = c[RC_MBASE],
                           cbase = c[RC_CBASE], ndisc = c[RC_NDISC], nmeth = c[RC_NMETH], nu = c[RC_NU], nx = c[RC_NX], nm = c[RC_NM];
  if ((nreads | nlong | kreads | tbase | mbase | cbase | ndisc | nmeth | nu | nx | nm) > 0x7FFFFFFFull) atomicMax(bad, (uint32_t)t + 1u);
  o.icol[0][t] = chr[t]; o.icol[1][t] = rs[t]; o.icol[2][t] = re[t];
  o.icol[3][t] = (int32_t)nreads; o.icol[4][t] = (int32_t)nlong; o.icol[5][t] = (int32_t)kreads; o.icol[6][t] = (int32_t)tbase;
  o.icol[7][t] = (int32_t)mbase; o.icol[8][t] = (int32_t)cbase; o.icol[9][t] = (int32_t)ndisc; o.icol[10][t] = (int32_t)nmeth;
  o.icol[11][t] = (int32_t)nu; o.icol[12][t] = (int32_t)nx; o.icol[13][t] = (int32_t)nm; o.icol[14][t] = maxsites;
  o.dcol[0][t] = rgn_ratio(mbase, tbase);
  o.dcol[1][t] = rgn_ratio(ndisc, kreads);
  o.dcol[2][t] = rgn_ratio(nmeth, kreads);
  o.dcol[3][t] = rgn_ratio(cbase, tbase);
  double mbs = 0.0;
  for (int32_t n = min_sites; n <= maxsites; n++) mbs += (double)S2[n] / (double)(n * n);     // ascending n
  o.dcol[4][t] = kreads ? mbs / (double)kreads : (double)NAN;
  // M[l] and T[l] in ascending l: M[l + 1] = M[l] - (runs of length >= l), T[l + 1] = T[l] - (counted rows with n >= l)
  unsigned long long M = 0, runs = 0, T = 0, rows = 0;
  for (int32_t l = 1; l <= maxsites; l++) { M += (unsigned long long)l * R[l]; runs += R[l]; T += (unsigned long long)l * H[l]; rows += H[l]; }
  double acc = 0.0;
  for (int32_t l = 1; l <= maxsites; l++) {
    acc += (double)l * ((double)M / (double)T);
    M -= runs; runs -= R[l];
    T -= rows; rows -= H[l];
  }
  o.dcol[5][t] = maxsites ? acc / (double)(maxsites * (maxsites + 1) / 2) : (double)NAN;
}

// the counters of nregions regions in bytes, or -1 outside 0 <= nregions < 2^31, 1 <= max_sites <= 256
static int64_t rgn_counter_bytes(int64_t nregions, int32_t max_sites) {
  if (nregions < 0 || nregions > 0x7FFFFFFFLL || max_sites < 1 || max_sites > kRgnMaxSites) return -1;
  return nregions * (int64_t)(RGN_HDR + 3 * max_sites) * 8;
}

struct RgnCall {
  const int32_t *d_chr, *d_start, *d_end;
  int32_t nregions, min_sites, max_sites, reverse_offset;
  const char *ctx;
  double u_max, m_min, max_oo;
  RgnOut out;
};

static int rgn_report(epi_batch *b, const RgnCall &c, hipStream_t s) {
  const char *who = "epi_batch_region_report_dev";
  const int32_t nt = c.nregions;
  int64_t lmax = 0;
  if (b->n > 0) {
    EPI_TRY(fetch_row_stats(b, s));
    if (b->h_stats.bad_len) return fail(EPI_ERR_ARG, "offsets are not non-decreasing, or start+length exceeds int32");
    if (b->h_stats.unsorted) return fail(EPI_ERR_UNSORTED, "PRE-SORTED DATASET IS A REQUIREMENT: rows are not sorted by (rname, start)");
    lmax = b->h_stats.max_len;
  }
  DevBuf d_rng, d_meta, d_cnt, d_bad;                         // the call's scratch: goes with it on every return path
  EPI_TRY(d_bad.ensure(sizeof(uint32_t)));
  EPI_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), s));
  const int64_t nbt = ((int64_t)nt + 255) / 256;
  EPI_TRY(check_grid(nbt, 256, who));

  // (a) the candidate rows of every region
  std::vector<int64_t> h_rng((size_t)2 * nt, 0);
  if (b->n > 0) {
    EPI_TRY(d_rng.ensure(h_rng.size() * 8));
    prof_begin("region_report", s);
    hipLaunchKernelGGL(k_rgn_ranges, dim3((unsigned)nbt), dim3(256), 0, s, b->rname, b->start, b->n, c.d_chr, c.d_start, c.d_end, nt, lmax,
                       (int64_t)c.reverse_offset, d_rng.as<int64_t>());
    EPI_HIP(hipGetLastError());
    prof_end("region_report", s);
    EPI_HIP(hipMemcpyAsync(h_rng.data(), d_rng.p, h_rng.size() * 8, hipMemcpyDeviceToHost, s));
    EPI_HIP(hipStreamSynchronize(s));
  }

  RgnArgs a;
  a.xm = b->xm; a.off = b->off; a.len = b->len; a.strand = b->strand; a.start = b->start;
  a.stride = (uint32_t)(RGN_HDR + 3 * c.max_sites);
  a.ctx_mask = ctx_mask_of(c.ctx);
  ooctx_masks(a.ctx_mask, &a.oom_mask, &a.oou_mask);
  a.min_sites = c.min_sites; a.max_sites = c.max_sites; a.reverse_offset = c.reverse_offset;
  a.u_max = c.u_max; a.m_min = c.m_min; a.max_oo = c.max_oo;
  const bool wide = b->nbytes > kSiteLongRow * b->n;           // long rows: a whole wave per pair
  const int64_t ngrp = wide ? RGN_WG / 64 : RGN_WG / 16;      // pairs a workgroup walks at a time

  // (b) - (d) group by group
  const int64_t cap = options().rgn_group_bytes > 0 ? options().rgn_group_bytes : kRgnGroupBytes;
  const int64_t per_region = (int64_t)a.stride * 8 + 16;      // its counters, pre[] and row_lo[]
  std::vector<std::vector<uint64_t>> metas;                   // what the uploads read: alive until the last synchronisation
  for (int32_t ta = 0; ta < nt;) {
    int32_t tb = ta + 1;
    while (tb < nt && (int64_t)(tb - ta + 1) * per_region <= cap) tb++;
    const int32_t ng = tb - ta;
    metas.emplace_back((size_t)(ng + 1) + (size_t)ng, 0);     // pre[ng + 1], row_lo[ng]
    uint64_t *pre = metas.back().data();
    int64_t *row_lo = reinterpret_cast<int64_t *>(pre + ng + 1);
    for (int32_t k = 0; k < ng; k++) {
      const size_t t = (size_t)(ta + k);
      row_lo[k] = h_rng[2 * t];
      pre[k + 1] = pre[k] + (uint64_t)(h_rng[2 * t + 1] - h_rng[2 * t]);
    }
    const uint64_t P = pre[ng];
    const size_t cbytes = (size_t)ng * a.stride * 8;
    EPI_TRY(d_meta.ensure(metas.back().size() * 8));
    EPI_TRY(d_cnt.ensure(cbytes));
    EPI_HIP(hipMemcpyAsync(d_meta.p, pre, metas.back().size() * 8, hipMemcpyHostToDevice, s));
    EPI_HIP(hipMemsetAsync(d_cnt.p, 0, cbytes, s));
    a.pre = d_meta.as<uint64_t>();
    a.row_lo = reinterpret_cast<const int64_t *>(d_meta.as<uint64_t>() + ng + 1);
    a.rs = c.d_start + ta; a.re = c.d_end + ta;
    a.cnt = d_cnt.as<unsigned long long>();
    a.npairs = P; a.ng = ng;
    prof_begin("region_report", s);
    if (P > 0) {
      // few pairs: short chunks, so that a list of shallow regions is spread over the device instead of being walked segment
      // by segment in a handful of workgroups; many: chunks of up to RGN_ROUNDS rounds, one flush each
      const uint64_t want = (P + (uint64_t)(ngrp * RGN_BLOCKS) - 1) / (uint64_t)(ngrp * RGN_BLOCKS);
      a.rounds = (uint32_t)(want < 1 ? 1 : want > (uint64_t)RGN_ROUNDS ? (uint64_t)RGN_ROUNDS : want);
      const uint64_t chunk = (uint64_t)ngrp * a.rounds;
      const int64_t nb = (int64_t)((P + chunk - 1) / chunk);
      EPI_TRY(check_grid(nb, RGN_WG, who));
      prof_begin("region_count", s);
      if (wide) hipLaunchKernelGGL((k_rgn_count<64>), dim3((unsigned)nb), dim3(RGN_WG), 0, s, a);
      else hipLaunchKernelGGL((k_rgn_count<16>), dim3((unsigned)nb), dim3(RGN_WG), 0, s, a);
      prof_end("region_count", s);
    }
    hipLaunchKernelGGL(k_rgn_finish, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, s, a.cnt, a.stride, ng, ta, c.d_chr, c.d_start, c.d_end,
                       c.min_sites, c.max_sites, c.out, d_bad.as<uint32_t>());
    EPI_HIP(hipGetLastError());
    prof_end("region_report", s);
    ta = tb;
  }
  uint32_t bad = 0;
  EPI_TRY(read_scalars(b, s, d_bad.p, sizeof(bad), &bad));
  if (bad) return fail(EPI_ERR_ARG, "%s: region %u has a count above 2^31 - 1, which an int32 column cannot hold", who, bad - 1u);
  return EPI_OK;
}

}  // namespace epi

using namespace epi;

extern "C" {

int epi_region_counter_bytes(int64_t nregions, int32_t max_sites, int64_t *bytes_out) {
  if (!bytes_out) return fail(EPI_ERR_ARG, "epi_region_counter_bytes: NULL argument");
  *bytes_out = 0;
  const int64_t bytes = rgn_counter_bytes(nregions, max_sites);
  if (bytes < 0)
    return fail(EPI_ERR_ARG, "epi_region_counter_bytes: %lld regions of max_sites = %d, 0 to 2^31 - 1 regions of 1 to %d sites", (long long)nregions,
                max_sites, kRgnMaxSites);
  *bytes_out = bytes;
  return EPI_OK;
}

int epi_batch_region_report_dev(epi_batch *b, const int32_t *d_chr, const int32_t *d_start, const int32_t *d_end, int32_t nregions,
                                const char *ctx, int32_t min_sites, int32_t max_sites, int32_t reverse_offset, double u_max, double m_min,
                                double max_ooctx_meth_frac, int32_t *const d_icols[15], double *const d_dcols[6], void *stream) {
  const char *who = "epi_batch_region_report_dev";
  if (!b) return fail(EPI_ERR_ARG, "%s: batch is NULL", who);
  if (!ctx) return fail(EPI_ERR_ARG, "%s: ctx is NULL", who);
  if (nregions < 0) return fail(EPI_ERR_ARG, "%s: nregions = %d is negative", who, nregions);
  if (max_sites < 1 || max_sites > kRgnMaxSites) return fail(EPI_ERR_ARG, "%s: max_sites = %d, a read is counted with 1 to %d sites", who, max_sites, kRgnMaxSites);
  if (min_sites < 1 || min_sites > max_sites) return fail(EPI_ERR_ARG, "%s: min_sites = %d, 1 to max_sites = %d", who, min_sites, max_sites);
  if (reverse_offset < 0) return fail(EPI_ERR_ARG, "%s: negative reverse_offset", who);
  if (!(u_max >= 0.0 && u_max < m_min && m_min <= 1.0)) return fail(EPI_ERR_ARG, "%s: u_max = %g and m_min = %g, 0 <= u_max < m_min <= 1", who, u_max, m_min);
  if (nregions > 0) {
    if (!d_chr || !d_start || !d_end) return fail(EPI_ERR_ARG, "%s: d_chr, d_start or d_end is NULL", who);
    if (!d_icols || !d_dcols) return fail(EPI_ERR_ARG, "%s: d_icols or d_dcols is NULL", who);
    for (int i = 0; i < 15; i++) if (!d_icols[i]) return fail(EPI_ERR_ARG, "%s: d_icols[%d] is NULL", who, i);
    for (int i = 0; i < 6; i++) if (!d_dcols[i]) return fail(EPI_ERR_ARG, "%s: d_dcols[%d] is NULL", who, i);
  }
  if (nregions == 0) return EPI_OK;
  EPI_HIP(hipSetDevice(b->eng->device));
  RgnCall c;
  c.d_chr = d_chr; c.d_start = d_start; c.d_end = d_end; c.nregions = nregions;
  c.min_sites = min_sites; c.max_sites = max_sites; c.reverse_offset = reverse_offset;
  c.ctx = ctx; c.u_max = u_max; c.m_min = m_min; c.max_oo = max_ooctx_meth_frac;
  for (int i = 0; i < 15; i++) c.out.icol[i] = d_icols[i];
  for (int i = 0; i < 6; i++) c.out.dcol[i] = d_dcols[i];
  return rgn_report(b, c, pick_stream(b, stream));
}

}  // extern "C"
