// Allele-specific methylation report: does methylation differ between the two alleles of a heterozygous SNV?  Per (SNV,
// cytosine) the calls of the reads that carry the reference allele against those of the reads that carry the alternative one
// (what CGmapTools asm, MethPipe allelicmeth and DAMEfinder's SNP mode report), and the same pooled per SNV.  The packed
// SEQXM byte holds the base (nt16 << 4) next to the call, so one row says both.  No reference interface is replaced;
// include/epihip.h, epi_batch_asm_report_dev, has the interface.
//
// Definitions.  ctx: context letters in both cases; max_oo = max_ooctx_meth_frac; D = max_distance; mc = max(min_coverage, 1).
//  Sites       nsite sites (site_chr: rname factor codes, INT32_MIN = NA; site_pos: 1-based; site_alleles), sorted by
//              (code, pos) with equal keys allowed (multi-ALT records) -- the precondition of epi_batch_base_freqs_dev, NA
//              codes (which sort first) included.  site_alleles: four 4-bit masks over the bases A, C, G, T (bit =
//              seq_nt16_int, 0 .. 3): bits 0-3 REF on '+' rows, 4-7 ALT on '+', 8-11 REF on '-', 12-15 ALT on '-'.  A zero
//              mask: the strand cannot tell the alleles apart.  A bit above 15, or REF and ALT of one strand sharing a bit,
//              is an error.
//  Kept rows   row x is kept by the lMHL read rule with hmin = 0 over the whole row (rcpp_mhl_report.cpp:172-179; the verdict
//              of xm_codes.hpp): o_m / (o_m + o_u) > max_oo drops it, o_m / o_u = its methylated (codes 2, 5, 6, 7) /
//              unmethylated (10, 13, 14, 15) bytes whose code is not one of ctx's; 0 / 0 is NaN and keeps the row.  Its
//              strand must be 1 or 2, its length positive, its rname not NA.
//  Allele      a kept row x COVERS site s when rname[x] == site_chr[s] and start[x] <= site_pos[s] <= start[x] + len[x] - 1
//              (an NA site is covered by no row).  Its base there is seq_nt16_int[byte >> 4] (base_freqs.hip); its allele is
//              0 (REF) when the base's bit is in its strand's REF mask, 1 (ALT) when in the ALT mask, none otherwise: N, the
//              0xF? filler between mates, a third base, an uninformative strand.
//  Events      for a covering row with an allele, every byte i of the row whose code is one of ctx's, at position
//              q = start[x] + i, with q != site_pos[s] and, when D > 0, |q - site_pos[s]| <= D (D == 0: no limit), is one
//              event (s, strand[x], q, context code = code & 7, allele, methylated = code < 8).
//  Pair rows   events grouped by (s, q, strand, context code); four cells meth_ref, unmeth_ref, meth_alt, unmeth_alt.  A group
//              is reported when meth_ref + unmeth_ref >= mc and meth_alt + unmeth_alt >= mc, in ascending (s, q, strand,
//              context).  Ten int32: snv (index into the site list as given), rname, snv_pos, strand, pos (= q), context, the
//              four cells.  Four double: beta_ref = meth_ref / (meth_ref + unmeth_ref), beta_alt likewise (one IEEE division
//              of integers each), delta_beta = beta_alt - beta_ref, p = fisher::fisher_two_sided(meth_ref, unmeth_ref,
//              meth_alt, unmeth_alt) by one thread per row, the function epi_fisher_exact_dev runs.
//  SNV rows    one per site, in input order.  Ten int32: rname, pos (as given), reads_ref, reads_alt, reads_other (kept
//              covering rows by allele / without one), npairs (the site's reported pair rows), and meth_ref, unmeth_ref,
//              meth_alt, unmeth_alt summed over the site's REPORTED pair rows: the SNV table is a group-by of the pair table.
//              Four double: beta_ref, beta_alt, delta_beta and p from the pooled cells; a zero denominator gives NaN (p of an
//              all-zero table is 1).  An NA site: zero counts and four NaN.  Sums are kept in 64 bits; one above 2^31 - 1 is
//              an error that names the site.
//
// Data path, all on the call's stream.
//  (a) k_asm_check_sites: order and masks of the sites; the verdict comes to the host (first synchronisation).
//  (b) k_asm_rows: the read rule, 16 lanes per row, 16 bytes per lane and step, the classes by a 16-entry byte LUT looked up
//      with three v_perm_b32 per dword (the scheme of per_read.hip) and popcounts: keep[x].
//  (c) k_asm_walk<false>: a workgroup owns 256 consecutive rows, finds its window of the sorted sites by two wavefront searches
//      (site_search.hpp, shared with k_base_freqs) and numbers the (row, site) pairs by a block scan.  The pairs are taken 256
//      at a time, one per thread: one byte load decides the allele and adds to the site's three read counters.  The pairs with
//      an allele are then cut into UNITS of one 16-byte chunk of the row each (only the chunks within D of the site), numbered
//      by a second block scan and dealt to the threads: a 10 kb row under a dense site list, or a 5000-deep pile-up on one
//      SNV, keeps every lane busy.  A unit is one 16-byte load, the LUT, a 16-bit mask of its eligible bytes and a popcount,
//      added to the site's event counter.  Counters are privatised in LDS while the window holds at most 256 sites (one global
//      atomic per non-zero counter at the end), else added in global memory.  The event counts come to the host (second
//      synchronisation), which forms the groups.
//  (d) Consecutive sites form a GROUP while their events (24 bytes each: the key and the sort's second buffers) stay under the
//      cap (256 MiB; EPIHIP_ASM_GROUP_BYTES; a site above it runs alone; a site with more than 2^31 - 1 events is an error).
//      Per group, k_asm_walk<true> repeats the walk over the group's sites and writes one 64-bit key per event:
//        site in the group << S | (q - site_pos + R) << 6 | (strand - 1) << 5 | context << 2 | cell
//      with cell = 2 allele + (methylated ? 0 : 1), R = the longest row (or D + 1 when that is smaller) and S = 6 + the bits of
//      2 R.  A unit batch reserves its events' places with one atomic add of the workgroup on the group's cursor; where an
//      event lands does not matter, the sort puts it in place and equal keys are only counted.
//  (e) radix_sort.hip's sort, in a SortPairs workspace, over the key bytes in use.
//  (f) k_asm_mark: a thread per event; the first event of a (site, q, strand, context) run finds the ends of the run's four
//      cell runs by galloping search -- the cells are lengths of runs of equal keys, no counter array and no atomics -- and
//      flags the run when both alleles have mc calls.  util.hip's scan turns the flags into output rows; their number comes to
//      the host (the group's synchronisation) and sizes the group's piece of the pair table, kept on the batch
//      (AsmState, common.hpp).  k_asm_write fills the piece's ten integer columns and adds the cells to the site's pooled sums.
//  (g) k_asm_snv: a thread per site writes the SNV columns; the overflow verdict is the last synchronisation.
//  Fetch: k_asm_fetch, a thread per pair row, copies the integer columns and computes the four doubles.
// Departure from "count per pair, scan, emit at the scanned offsets": no pair list is materialised (its length is bounded only
// by rows x sites); places come from a cursor instead, which the sort makes irrelevant to the result.  Allele and state ride
// in the key's two lowest bits instead of in the sort's 32-bit value (zero-filled here), so that the cells can be read off
// the sorted keys.  Every reported number is an integer count or computed from integer counts by one thread in a fixed order.
#include <math.h>
#include <string.h>
#include <vector>
#include "radix_sort.hpp"
#include "site_search.hpp"
#include "fisher_math.hpp"

namespace epi {

constexpr int ASM_WG = 256;                         // rows (= threads) per workgroup of the walk
constexpr int ASM_CAP = 256;                        // window sites counted in LDS
constexpr int64_t kAsmGroupBytes = 256LL << 20;
constexpr uint32_t kAsmNoSite = 0xFFFFFFFFu;

struct AsmScalars {                                 // what the kernels and the host exchange (64 bytes allocated)
  uint32_t unsorted;                                // the sites are not in (code, pos) order
  uint32_t bad_site;                                // first site with a bad allele mask (kAsmNoSite: none)
  uint32_t overflow;                                // an event had no place left (the count and the emit walk disagree)
  uint32_t nkept;                                   // reported pair rows of the group
  unsigned long long cursor;                        // events written by the group's emit walk
  uint32_t bad_sum;                                 // 1 + the last site with a count above int32
  uint32_t unused;
};
static_assert(sizeof(AsmScalars) == 32 && offsetof(AsmScalars, cursor) == 16, "AsmScalars layout");

// LUT byte of a code: bit 0 one of ctx's, bit 1 ... and methylated, bit 2 / 3 out-of-context methylated / unmethylated
static ClassLut asm_make_lut(uint32_t ctx_mask) {
  uint8_t f[16];
  for (uint32_t c = 0; c < 16; c++) {
    if ((ctx_mask >> c) & 1u) f[c] = 1u | (c < 8u ? 2u : 0u);
    else f[c] = ((kXmMethMask >> c) & 1u ? 4u : 0u) | ((kXmUnmethMask >> c) & 1u ? 8u : 0u);
  }
  return lut16_pack(f);
}

// 16 bytes from p, of which the first `avail` belong to the row; the rest read as '.' (code 12: in no class)
__device__ __forceinline__ uint4 asm_load16(const uint8_t *__restrict__ p, int64_t avail) {
  uint4 w;
  if (avail >= 16) { memcpy(&w, p, 16); return w; }
  uint64_t lo = ((uint64_t)kXmDot4 << 32) | kXmDot4, hi = lo;
  for (int j = 0; j < (int)avail; j++) {
    const uint64_t v = p[j];
    if (j < 8) lo = (lo & ~(0xFFull << (8 * j))) | (v << (8 * j));
    else hi = (hi & ~(0xFFull << (8 * (j - 8)))) | (v << (8 * (j - 8)));
  }
  w.x = (uint32_t)lo; w.y = (uint32_t)(lo >> 32); w.z = (uint32_t)hi; w.w = (uint32_t)(hi >> 32);
  return w;
}

__global__ __launch_bounds__(256) void k_asm_check_sites(const int32_t *__restrict__ chr, const int32_t *__restrict__ pos,
                                                         const int32_t *__restrict__ all, int64_t n, AsmScalars *__restrict__ sc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (i > 0 && site_key(chr[i], pos[i]) < site_key(chr[i - 1], pos[i - 1])) atomicOr(&sc->unsorted, 1u);
  const uint32_t m = (uint32_t)all[i];
  if ((m >> 16) != 0u || (m & (m >> 4) & 0x0F0Fu) != 0u) atomicMin(&sc->bad_site, (uint32_t)i);
}

// (b) the read rule: 16 lanes per row
__global__ __launch_bounds__(ASM_WG) void k_asm_rows(const uint8_t *__restrict__ xm, const int64_t *__restrict__ off, const int32_t *__restrict__ len,
                                                     const int32_t *__restrict__ rname, const int32_t *__restrict__ strand, int64_t n, ClassLut F,
                                                     double max_oo, uint8_t *__restrict__ keep) {
  const uint32_t sub = threadIdx.x & 15u;
  const int64_t row = (int64_t)blockIdx.x * (ASM_WG / 16) + (threadIdx.x >> 4);
  const bool have = row < n;
  const int32_t st = have ? strand[row] : 0;
  const int32_t l = have && (st == 1 || st == 2) && rname[row] != INT32_MIN ? len[row] : 0;
  const uint8_t *p = xm + (have ? off[row] : 0);
  uint32_t om = 0, ou = 0;
  for (int64_t c = (int64_t)sub * 16; c < l; c += 256) {
    const uint4 w = asm_load16(p + c, (int64_t)l - c);
    const uint32_t r0 = lut16_pick(w.x, F), r1 = lut16_pick(w.y, F), r2 = lut16_pick(w.z, F), r3 = lut16_pick(w.w, F);
    om += (uint32_t)(__popc(r0 & 0x04040404u) + __popc(r1 & 0x04040404u) + __popc(r2 & 0x04040404u) + __popc(r3 & 0x04040404u));
    ou += (uint32_t)(__popc(r0 & 0x08080808u) + __popc(r1 & 0x08080808u) + __popc(r2 & 0x08080808u) + __popc(r3 & 0x08080808u));
  }
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) { om += __shfl_xor(om, d, 64); ou += __shfl_xor(ou, d, 64); }
  if (have && sub == 0) keep[row] = read_rule_keeps(l, om, ou, max_oo) ? 1 : 0;
}

struct AsmArgs {
  const uint8_t *xm;
  const int64_t *off;
  const int32_t *len, *rname, *strand, *start;
  const uint8_t *keep;
  int64_t n;
  const int32_t *s_chr, *s_pos, *s_all;   // the sites the walk is over: all of them when counting, the group's when emitting
  int64_t nsite;
  ClassLut lut;
  int32_t max_dist, R;
  uint32_t sshift;
  uint32_t *reads;                        // count: [3][nsite] kept covering rows by allele
  unsigned long long *events;             // count: [nsite]
  uint64_t *key;                          // emit: [cap]
  uint64_t cap;
  AsmScalars *sc;
};

// the last r in [0, ASM_WG) with s[r] <= j (s ascends, s[ASM_WG] > j: entry r holds item j)
__device__ __forceinline__ int32_t asm_owner(const unsigned long long *s, uint64_t j) {
  int32_t a = 0, b = ASM_WG;
  while (b - a > 1) { const int32_t m = (a + b) >> 1; if (s[m] <= j) a = m; else b = m; }
  return a;
}

// (c), (d) the walk over the (row, site) pairs of 256 rows: EMIT = false counts, EMIT = true writes the events' keys
template <bool EMIT>
__global__ __launch_bounds__(ASM_WG) void k_asm_walk(AsmArgs a) {
  __shared__ int64_t wkey[ASM_CAP];
  __shared__ uint32_t cnt[3 * ASM_CAP];               // [allele or none][window site]
  __shared__ unsigned long long ev[ASM_CAP];
  __shared__ unsigned long long pre[ASM_WG + 1];              // pairs of the rows before row t
  __shared__ unsigned long long upre[ASM_WG + 1];              // units of the batch's pairs before pair t
  __shared__ unsigned long long epre[ASM_WG + 1];              // events of the round's units before unit t
  __shared__ unsigned long long wsum[ASM_WG / 64];
  __shared__ int64_t r_off[ASM_WG];
  __shared__ int32_t r_lo[ASM_WG], r_start[ASM_WG], r_len[ASM_WG], r_sd[ASM_WG];
  __shared__ int32_t p_row[ASM_WG], p_site[ASM_WG], p_al[ASM_WG];
  __shared__ int64_t p_ip[ASM_WG];                    // the site's byte in the row
  __shared__ uint32_t p_c0[ASM_WG];                   // the pair's first chunk
  __shared__ int64_t red_min[ASM_WG / 64], red_max[ASM_WG / 64], win[2];
  __shared__ unsigned long long s_base;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int64_t x = (int64_t)blockIdx.x * ASM_WG + t;
  int32_t rc = 0, st = 0, l = 0, sd = 0;
  bool valid = false;
  if (x < a.n && a.keep[x]) { rc = a.rname[x]; st = a.start[x]; l = a.len[x]; sd = a.strand[x]; valid = l > 0; }   // (keep: strand 1 / 2)
  const int64_t k_lo = valid ? site_key(rc, st) : INT64_MAX;
  const int64_t k_hi = valid ? site_key(rc, st) + l : INT64_MIN;     // key of (rname, end + 1)

  // the window of sites the workgroup's rows can touch
  int64_t mn = k_lo, mx = k_hi;
  for (int d = 32; d >= 1; d >>= 1) {
    const int64_t u = __shfl_xor(mn, d, 64), v = __shfl_xor(mx, d, 64);
    mn = u < mn ? u : mn;
    mx = v > mx ? v : mx;
  }
  if (lane == 0) { red_min[wave] = mn; red_max[wave] = mx; }
  __syncthreads();
  mn = red_min[0]; mx = red_max[0];
  for (int w = 1; w < ASM_WG / 64; w++) { mn = red_min[w] < mn ? red_min[w] : mn; mx = red_max[w] > mx ? red_max[w] : mx; }
  if (mx == INT64_MIN) return;                       // no kept row (uniform)
  if (wave < 2) {
    const int64_t r = wave_lower_bound(a.s_chr, a.s_pos, a.nsite, wave == 0 ? mn : mx);
    if (lane == 0) win[wave] = r;
  }
  __syncthreads();
  const int64_t lo = win[0], W = win[1] - win[0];
  if (W <= 0) return;
  const bool in_lds = W <= ASM_CAP;
  if (in_lds) {
    for (int i = t; i < (int)W; i += ASM_WG) wkey[i] = site_key(a.s_chr[lo + i], a.s_pos[lo + i]);
    if (!EMIT) {
      for (int i = t; i < 3 * ASM_CAP; i += ASM_WG) cnt[i] = 0;
      for (int i = t; i < ASM_CAP; i += ASM_WG) ev[i] = 0;
    }
    __syncthreads();
  }

  // each row's sites inside the window, and the pairs numbered by a block scan
  int64_t c_row = 0;
  if (valid) {
    int64_t s0, s1;
    if (in_lds) { s0 = lds_lower_bound(wkey, (int32_t)W, k_lo); s1 = lds_lower_bound(wkey, (int32_t)W, k_hi); }
    else { s0 = glb_lower_bound(a.s_chr, a.s_pos, lo, lo + W, k_lo) - lo; s1 = glb_lower_bound(a.s_chr, a.s_pos, lo + s0, lo + W, k_hi) - lo; }
    c_row = s1 - s0;
    r_lo[t] = (int32_t)s0;
    r_off[t] = a.off[x];
    r_start[t] = st; r_len[t] = l; r_sd[t] = sd;
  }
  wg_scan_table<SumU64, ASM_WG>((unsigned long long)c_row, pre, wsum);
  const uint64_t P = pre[ASM_WG];

  for (uint64_t pb = 0; pb < P; pb += ASM_WG) {          // 256 pairs, one per thread
    const uint64_t j = pb + t;
    unsigned long long nch = 0;
    if (j < P) {
      const int32_t r = asm_owner(pre, j);
      const int32_t site = r_lo[r] + (int32_t)(j - pre[r]);
      const int64_t ip = (int64_t)a.s_pos[lo + site] - r_start[r];       // 0 <= ip < len: the search's bounds
      const uint32_t nib = a.xm[r_off[r] + ip] >> 4;
      const uint32_t code = (uint32_t)((kNt16Int >> (4 * nib)) & 15u);
      const uint32_t bit = code < 4u ? 1u << code : 0u;
      const uint32_t m = (uint32_t)a.s_all[lo + site] >> (r_sd[r] == 2 ? 8 : 0);
      const int32_t al = (m & bit) ? 0 : ((m >> 4) & bit) ? 1 : 2;
      if (!EMIT) {
        if (in_lds) atomicAdd(&cnt[al * ASM_CAP + site], 1u);
        else atomicAdd(&a.reads[(int64_t)al * a.nsite + lo + site], 1u);
      }
      uint32_t c0 = 0;
      if (al < 2) {                                        // the row's chunks that hold a byte within max_dist of the site
        int64_t i0 = 0, i1 = r_len[r];
        if (a.max_dist > 0) {
          i0 = ip - a.max_dist > 0 ? ip - a.max_dist : 0;
          i1 = ip + a.max_dist + 1 < i1 ? ip + a.max_dist + 1 : i1;
        }
        c0 = (uint32_t)(i0 >> 4);
        nch = (uint64_t)(((i1 + 15) >> 4) - (i0 >> 4));    // (i1 > i0: byte ip is inside)
      }
      p_row[t] = r; p_site[t] = site; p_al[t] = al; p_ip[t] = ip; p_c0[t] = c0;
    }
    wg_scan_table<SumU64, ASM_WG>(nch, upre, wsum);
    const uint64_t U = upre[ASM_WG];

    for (uint64_t ub = 0; ub < U; ub += ASM_WG) {          // 256 units, one per thread
      const uint64_t u = ub + t;
      uint32_t elig = 0, site = 0, al = 0, sdm1 = 0;
      int64_t b0 = 0, ip = 0;
      uint4 w = make_uint4(0, 0, 0, 0);
      if (u < U) {
        const int32_t k = asm_owner(upre, u);
        const int32_t r = p_row[k];
        site = (uint32_t)p_site[k]; al = (uint32_t)p_al[k]; ip = p_ip[k]; sdm1 = (uint32_t)(r_sd[r] - 1);
        const int64_t len = r_len[r];
        b0 = ((int64_t)p_c0[k] + (int64_t)(u - upre[k])) << 4;            // the chunk's first byte in the row: < len
        w = asm_load16(a.xm + r_off[r] + b0, len - b0);
        int64_t i0 = 0, i1 = len;
        if (a.max_dist > 0) {
          i0 = ip - a.max_dist > 0 ? ip - a.max_dist : 0;
          i1 = ip + a.max_dist + 1 < i1 ? ip + a.max_dist + 1 : i1;
        }
        const int64_t e0 = i0 - b0, e1 = i1 - b0, es = ip - b0;
        const uint32_t m0 = e0 <= 0 ? 0u : e0 >= 16 ? 16u : (uint32_t)e0, m1 = e1 <= 0 ? 0u : e1 >= 16 ? 16u : (uint32_t)e1;
        uint32_t rm = ((1u << m1) - 1u) & ~((1u << m0) - 1u);
        if (es >= 0 && es < 16) rm &= ~(1u << (uint32_t)es);              // q != site_pos
        const uint32_t r0 = lut16_pick(w.x, a.lut), r1 = lut16_pick(w.y, a.lut), r2 = lut16_pick(w.z, a.lut), r3 = lut16_pick(w.w, a.lut);
        elig = (plane_nibble_mul(r0, 0) | (plane_nibble_mul(r1, 0) << 4) | (plane_nibble_mul(r2, 0) << 8) | (plane_nibble_mul(r3, 0) << 12)) & rm;
      }
      const uint32_t ne = (uint32_t)__popc(elig);
      if (!EMIT) {
        // one add per wavefront when its units are all of one site (a pile-up), else one per unit with an event
        const unsigned long long act = __ballot(ne != 0u);
        if (act != 0ull) {
          const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)site, __ffsll((long long)act) - 1);
          if (__all(ne == 0u || site == first)) {
            const uint32_t tot = wave_sum_u32(ne);
            if (lane == 0) {
              if (in_lds) atomicAdd(&ev[first], (unsigned long long)tot);
              else atomicAdd(&a.events[lo + first], (unsigned long long)tot);
            }
          } else if (ne) {
            if (in_lds) atomicAdd(&ev[site], (unsigned long long)ne);
            else atomicAdd(&a.events[lo + site], (unsigned long long)ne);
          }
        }
      } else {
        wg_scan_table<SumU64, ASM_WG>((unsigned long long)ne, epre, wsum);
        const uint64_t total = epre[ASM_WG];
        if (total) {                                           // (uniform)
          if (t == 0) s_base = atomicAdd(&a.sc->cursor, (unsigned long long)total);
          __syncthreads();
          uint64_t at = s_base + epre[t];
          const uint64_t hi = ((uint64_t)(lo + site) << a.sshift) | ((uint64_t)sdm1 << 5);
          uint32_t e = elig;
          while (e) {
            const uint32_t jb = (uint32_t)__ffs((int)e) - 1u;
            e &= e - 1u;
            const uint32_t wd = jb < 4u ? w.x : jb < 8u ? w.y : jb < 12u ? w.z : w.w;
            const uint32_t nib = (wd >> (8u * (jb & 3u))) & 15u;
            const uint64_t dq = (uint64_t)(b0 + jb - ip + a.R);            // q - site_pos + R, in [1, 2 R)
            const uint64_t key = hi | (dq << 6) | ((uint64_t)(nib & 7u) << 2) | (uint64_t)(2u * al + (nib < 8u ? 0u : 1u));
            if (at < a.cap) a.key[at] = key;
            else atomicOr(&a.sc->overflow, 1u);
            at++;
          }
        }
      }
    }
    __syncthreads();                                       // the next batch's pairs replace p_*: every unit of this one has read them
  }
  if (EMIT || !in_lds) return;
  __syncthreads();
  for (int i = t; i < 3 * (int)W; i += ASM_WG) {
    const int c = i / (int)W, site = i - c * (int)W;
    const uint32_t v = cnt[c * ASM_CAP + site];
    if (v) atomicAdd(&a.reads[(int64_t)c * a.nsite + lo + site], v);
  }
  for (int i = t; i < (int)W; i += ASM_WG) {
    const unsigned long long v = ev[i];
    if (v) atomicAdd(&a.events[lo + i], v);
  }
}

// ---- (f) reduce -----------------------------------------------------------------------------------------------------------

// first index in [i, n) whose key is >= target (the keys ascend): gallop from i, then bisect
__device__ __forceinline__ uint64_t asm_run_end(const uint64_t *__restrict__ key, uint64_t i, uint64_t n, uint64_t target) {
  if (i >= n || key[i] >= target) return i;
  uint64_t below = i, step = 1;                          // key[below] < target
  while (below + step < n && key[below + step] < target) { below += step; step <<= 1; }
  uint64_t a = below + 1, b = below + step < n ? below + step : n;   // the answer is in [a, b]
  while (a < b) { const uint64_t m = a + ((b - a) >> 1); if (key[m] < target) a = m + 1; else b = m; }
  return a;
}

// the four cells of the run of (site, q, strand, context) = g that starts at event i
__device__ __forceinline__ void asm_cells(const uint64_t *__restrict__ key, uint64_t i, uint64_t n, uint64_t g, uint32_t c[4]) {
  uint64_t e = i;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const uint64_t nx = asm_run_end(key, e, n, v < 3 ? (g << 2) | (uint64_t)(v + 1) : (g + 1) << 2);
    c[v] = (uint32_t)(nx - e);
    e = nx;
  }
}

__global__ __launch_bounds__(ASM_WG) void k_asm_mark(const uint64_t *__restrict__ key, uint32_t n, uint32_t mc, uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * (uint32_t)ASM_WG + threadIdx.x;
  if (i >= n) return;
  const uint64_t g = key[i] >> 2;
  uint32_t f = 0;
  if (i == 0 || (key[i - 1] >> 2) != g) {
    uint32_t c[4];
    asm_cells(key, i, n, g, c);
    f = (uint64_t)c[0] + c[1] >= mc && (uint64_t)c[2] + c[3] >= mc ? 1u : 0u;
  }
  flag[i] = f;
}

struct AsmWrite {
  const uint64_t *key;
  const uint32_t *flag, *out;
  uint32_t n, nrow;                       // events; rows of the piece
  int32_t *piece;                         // [10][nrow]
  const int32_t *s_chr, *s_pos;           // all sites
  int64_t site0, nsite;                   // the group's first site
  uint32_t sshift;
  int32_t R;
  unsigned long long *pooled;             // [4][nsite]
  uint32_t *npairs;                       // [nsite]
};

__global__ __launch_bounds__(ASM_WG) void k_asm_write(AsmWrite a) {
  const uint32_t i = blockIdx.x * (uint32_t)ASM_WG + threadIdx.x;
  if (i >= a.n || !a.flag[i]) return;
  const uint32_t r = a.out[i];
  if (r >= a.nrow) return;
  const uint64_t g = a.key[i] >> 2;
  uint32_t c[4];
  asm_cells(a.key, i, a.n, g, c);
  const int64_t site = a.site0 + (int64_t)(a.key[i] >> a.sshift);
  const int32_t p = a.s_pos[site];
  const int64_t dq = (int64_t)((a.key[i] >> 6) & ((1ull << (a.sshift - 6u)) - 1ull));
  int32_t *o = a.piece + r;
  const size_t nr = a.nrow;
  o[0] = (int32_t)site; o[nr] = a.s_chr[site]; o[2 * nr] = p; o[3 * nr] = (int32_t)((g >> 3) & 1u) + 1;
  o[4 * nr] = (int32_t)((int64_t)p + dq - a.R); o[5 * nr] = (int32_t)(g & 7u);
#pragma unroll
  for (int v = 0; v < 4; v++) {
    o[(6 + v) * nr] = (int32_t)c[v];
    if (c[v]) atomicAdd(&a.pooled[(int64_t)v * a.nsite + site], (unsigned long long)c[v]);
  }
  atomicAdd(&a.npairs[site], 1u);
}

__device__ __forceinline__ double asm_ratio(unsigned long long a, unsigned long long b) { return b ? (double)a / (double)b : (double)NAN; }

struct AsmCols {
  int32_t *icol[10];
  double *dcol[4];
};

// (g) the SNV rows
__global__ __launch_bounds__(ASM_WG) void k_asm_snv(const int32_t *__restrict__ chr, const int32_t *__restrict__ pos, int64_t nsite,
                                                    const uint32_t *__restrict__ reads, const uint32_t *__restrict__ npairs,
                                                    const unsigned long long *__restrict__ pooled, AsmCols o, AsmScalars *__restrict__ sc) {
  const int64_t i = (int64_t)blockIdx.x * ASM_WG + threadIdx.x;
  if (i >= nsite) return;
  const int32_t c = chr[i];
  const unsigned long long m[4] = {pooled[i], pooled[nsite + i], pooled[2 * nsite + i], pooled[3 * nsite + i]};
  const uint32_t rd[3] = {reads[i], reads[nsite + i], reads[2 * nsite + i]}, np = npairs[i];
  if ((m[0] | m[1] | m[2] | m[3] | rd[0] | rd[1] | rd[2] | np) > 0x7FFFFFFFull) atomicMax(&sc->bad_sum, (uint32_t)i + 1u);
  o.icol[0][i] = c; o.icol[1][i] = pos[i];
  o.icol[2][i] = (int32_t)rd[0]; o.icol[3][i] = (int32_t)rd[1]; o.icol[4][i] = (int32_t)rd[2]; o.icol[5][i] = (int32_t)np;
#pragma unroll
  for (int v = 0; v < 4; v++) o.icol[6 + v][i] = (int32_t)m[v];
  const double br = asm_ratio(m[0], m[0] + m[1]), ba = asm_ratio(m[2], m[2] + m[3]);
  o.dcol[0][i] = br; o.dcol[1][i] = ba; o.dcol[2][i] = ba - br;
  o.dcol[3][i] = c == INT32_MIN ? (double)NAN : fisher::fisher_two_sided((int64_t)m[0], (int64_t)m[1], (int64_t)m[2], (int64_t)m[3]);
}

// fetch: rows [0, nrow) of a piece to rows row0 .. of the caller's columns
__global__ __launch_bounds__(ASM_WG) void k_asm_fetch(const int32_t *__restrict__ piece, int64_t nrow, int64_t row0, AsmCols o) {
  const int64_t i = (int64_t)blockIdx.x * ASM_WG + threadIdx.x;
  if (i >= nrow) return;
  int32_t v[10];
#pragma unroll
  for (int k = 0; k < 10; k++) { v[k] = piece[(int64_t)k * nrow + i]; o.icol[k][row0 + i] = v[k]; }
  const double br = (double)v[6] / (double)((int64_t)v[6] + v[7]), ba = (double)v[8] / (double)((int64_t)v[8] + v[9]);
  o.dcol[0][row0 + i] = br; o.dcol[1][row0 + i] = ba; o.dcol[2][row0 + i] = ba - br;
  o.dcol[3][row0 + i] = fisher::fisher_two_sided(v[6], v[7], v[8], v[9]);
}

// ---- host -------------------------------------------------------------------------------------------------------------------

static int64_t asm_event_bytes(int64_t nevents) { return nevents < 0 || nevents >= (1LL << 32) ? -1 : (int64_t)SortPairs::pair_bytes((size_t)nevents); }

struct AsmCall {
  const int32_t *d_chr, *d_pos, *d_all;
  int64_t nsite;
  const char *ctx;
  int32_t max_dist, min_cov;
  double max_oo;
  AsmCols snv;
};

struct AsmWork {                                    // the call's scratch (goes with it on every return path) and what its steps share
  DevBuf d_sc, d_cnt, d_keep, d_ev;
  AsmScalars *sc = nullptr;
  unsigned long long *d_events = nullptr, *d_pooled = nullptr;   // the sites' counters: events [ns] and pooled cells [4][ns] in 64 bits,
  uint32_t *d_reads = nullptr, *d_npairs = nullptr;              // ... reads [3][ns] and pair rows [ns] in 32
  AsmArgs a;                                        // the walk over all sites
  uint32_t qbits = 1;                               // q - site_pos + R < 2 R < 2^qbits
  int64_t nb_walk = 0;
};

// (a) the sites' order and masks (first synchronisation), then their zeroed counters
static int asm_sites(epi_batch *b, const AsmCall &c, AsmWork &w, hipStream_t s) {
  const char *who = "epi_batch_asm_report_dev";
  const int64_t ns = c.nsite, nb_sites = (ns + 255) / 256;
  EPI_TRY(w.d_sc.ensure(64));
  w.sc = w.d_sc.as<AsmScalars>();
  EPI_HIP(hipMemsetAsync(w.sc, 0, 64, s));
  EPI_HIP(hipMemsetAsync(&w.sc->bad_site, 0xFF, 4, s));
  EPI_TRY(check_grid(nb_sites, 256, who));
  hipLaunchKernelGGL(k_asm_check_sites, dim3((unsigned)nb_sites), dim3(256), 0, s, c.d_chr, c.d_pos, c.d_all, ns, w.sc);
  EPI_HIP(hipGetLastError());
  AsmScalars h;
  EPI_TRY(read_scalars(b, s, w.sc, sizeof(h), &h));
  if (h.bad_site != kAsmNoSite)
    return fail(EPI_ERR_ARG, "%s: d_site_alleles of site %u has a bit above 15, or REF and ALT of one strand share a base", who, h.bad_site);
  if (h.unsorted) return fail(EPI_ERR_UNSORTED, "VCF sites are not sorted by (seqnames, start)");
  EPI_TRY(w.d_cnt.ensure((size_t)ns * 56));
  EPI_HIP(hipMemsetAsync(w.d_cnt.p, 0, (size_t)ns * 56, s));
  w.d_events = w.d_cnt.as<unsigned long long>(); w.d_pooled = w.d_events + ns;
  w.d_reads = reinterpret_cast<uint32_t *>(w.d_pooled + 4 * ns); w.d_npairs = w.d_reads + 3 * ns;
  return EPI_OK;
}

// (b), (c) the read rule, then alleles, read counters and the events of every site: h_ev (second synchronisation), left
// empty when the batch has no byte to walk
static int asm_count(epi_batch *b, const AsmCall &c, AsmWork &w, hipStream_t s, std::vector<unsigned long long> &h_ev) {
  const char *who = "epi_batch_asm_report_dev";
  int64_t lmax = 0;
  if (b->n > 0) {
    EPI_TRY(fetch_row_stats(b, s));
    if (b->h_stats.bad_len) return fail(EPI_ERR_ARG, "offsets are not non-decreasing, or start+length exceeds int32");
    if (b->h_stats.unsorted) return fail(EPI_ERR_UNSORTED, "PRE-SORTED DATASET IS A REQUIREMENT: rows are not sorted by (rname, start)");
    lmax = b->h_stats.max_len;
  }
  if (lmax == 0) return EPI_OK;
  AsmArgs &a = w.a;
  a.xm = b->xm; a.off = b->off; a.len = b->len; a.rname = b->rname; a.strand = b->strand; a.start = b->start; a.n = b->n;
  a.lut = asm_make_lut(ctx_mask_of(c.ctx));
  a.max_dist = c.max_dist;
  const int64_t R = c.max_dist > 0 && (int64_t)c.max_dist + 1 < lmax ? (int64_t)c.max_dist + 1 : lmax;
  a.R = (int32_t)R;
  while ((2 * R) >> w.qbits) w.qbits++;
  a.sshift = 6u + w.qbits;
  a.reads = w.d_reads; a.events = w.d_events;
  a.key = nullptr; a.cap = 0; a.sc = w.sc;

  EPI_TRY(w.d_keep.ensure((size_t)b->n));
  a.keep = w.d_keep.as<uint8_t>();
  const int64_t nb_rule = (b->n + ASM_WG / 16 - 1) / (ASM_WG / 16);
  w.nb_walk = (b->n + ASM_WG - 1) / ASM_WG;
  EPI_TRY(check_grid(nb_rule, ASM_WG, who));
  EPI_TRY(check_grid(w.nb_walk, ASM_WG, who));
  prof_begin("asm_rows", s);
  hipLaunchKernelGGL(k_asm_rows, dim3((unsigned)nb_rule), dim3(ASM_WG), 0, s, b->xm, b->off, b->len, b->rname, b->strand, b->n, a.lut,
                     c.max_oo, w.d_keep.as<uint8_t>());
  prof_end("asm_rows", s);
  EPI_HIP(hipGetLastError());

  a.s_chr = c.d_chr; a.s_pos = c.d_pos; a.s_all = c.d_all; a.nsite = c.nsite;
  prof_begin("asm_count", s);
  hipLaunchKernelGGL((k_asm_walk<false>), dim3((unsigned)w.nb_walk), dim3(ASM_WG), 0, s, a);
  prof_end("asm_count", s);
  EPI_HIP(hipGetLastError());
  h_ev.resize((size_t)c.nsite);
  return copy_to_host(b->eng, h_ev.data(), w.d_events, (size_t)c.nsite * 8, s);
}

// (d) the grouping rule: the sites from ga on that form the next group -- while their events' (key, value) buffers stay under
// cap_bytes, they are at most max_sites and their events at most 2^31 - 1; a site beyond a limit runs alone (and beyond the
// last one is the caller's error).  Returns the group's end, *ne_out its events.
static int64_t asm_group_end(const std::vector<unsigned long long> &ev, int64_t ga, int64_t max_sites, int64_t cap_bytes,
                             unsigned long long *ne_out) {
  const int64_t ns = (int64_t)ev.size();
  unsigned long long ne = ev[ga];
  int64_t gb = ga + 1;
  while (gb < ns && gb - ga < max_sites && ne + ev[gb] <= 0x7FFFFFFFull && (int64_t)SortPairs::pair_bytes((size_t)(ne + ev[gb])) <= cap_bytes)
    ne += ev[gb++];
  *ne_out = ne;
  return gb;
}

// (f) the group's reported runs: a piece of the pair table of nkept rows and their cells added to the sites' pooled sums
static int asm_piece(epi_batch *b, const AsmCall &c, const AsmWork &w, const SortPairs &sort, size_t n, int64_t ga, uint32_t nkept,
                     hipStream_t s) {
  AsmState &st = b->asmr;
  st.piece.emplace_back();
  st.rows.push_back(0);                                       // (the piece is counted once it is written)
  EPI_TRY(st.piece.back().ensure((size_t)nkept * 40));
  AsmWrite wr;
  wr.key = sort.keys(); wr.flag = sort.spare<uint32_t>(); wr.out = wr.flag + n; wr.n = (uint32_t)n; wr.nrow = nkept;
  wr.piece = st.piece.back().as<int32_t>();
  wr.s_chr = c.d_chr; wr.s_pos = c.d_pos; wr.site0 = ga; wr.nsite = c.nsite;
  wr.sshift = w.a.sshift; wr.R = w.a.R;
  wr.pooled = w.d_pooled; wr.npairs = w.d_npairs;
  prof_begin("asm_reduce", s);
  hipLaunchKernelGGL(k_asm_write, dim3((unsigned)((n + ASM_WG - 1) / ASM_WG)), dim3(ASM_WG), 0, s, wr);
  prof_end("asm_reduce", s);
  EPI_HIP(hipGetLastError());
  st.rows.back() = nkept;
  return EPI_OK;
}

// (d) - (f) one group: sites [ga, gb) with ne > 0 events; the group's synchronisation
static int asm_group(epi_batch *b, const AsmCall &c, AsmWork &w, int64_t ga, int64_t gb, unsigned long long ne, hipStream_t s,
                     int64_t *npair) {
  const char *who = "epi_batch_asm_report_dev";
  const size_t n = (size_t)ne;
  const int64_t ng = gb - ga, nb_ev = ((int64_t)n + ASM_WG - 1) / ASM_WG;
  EPI_TRY(check_grid(nb_ev, ASM_WG, who));
  EPI_TRY(w.d_ev.ensure(SortPairs::bytes(n)));
  SortPairs sort(w.d_ev.p, n);
  EPI_HIP(hipMemsetAsync(sort.vals_in(), 0, n * 4, s));       // (the sort moves a value with every key; the report has none)
  EPI_HIP(hipMemsetAsync(&w.sc->overflow, 0, 16, s));         // overflow, nkept, cursor
  AsmArgs a = w.a;                                            // the walk over the group's sites
  a.s_chr = c.d_chr + ga; a.s_pos = c.d_pos + ga; a.s_all = c.d_all + ga; a.nsite = ng;
  a.key = sort.keys_in(); a.cap = n;
  prof_begin("asm_emit", s);
  hipLaunchKernelGGL((k_asm_walk<true>), dim3((unsigned)w.nb_walk), dim3(ASM_WG), 0, s, a);
  prof_end("asm_emit", s);
  EPI_HIP(hipGetLastError());

  // (e) the key bytes in use
  const uint64_t maxkey = ((uint64_t)(ng - 1) << a.sshift) | ((1ull << a.sshift) - 1ull);
  uint32_t bytes = 0;
  for (int d = 0; d < 8; d++) if (maxkey >> (8 * d)) bytes |= 1u << d;
  prof_begin("asm_sort", s);
  const int rc_sort = sort.sort(bytes, b->scan_tmp, s);
  prof_end("asm_sort", s);
  EPI_TRY(rc_sort);

  // (f) which runs are reported, and where (flags and rows in the sort's spare buffer)
  uint32_t *flag = sort.spare<uint32_t>(), *out = flag + n;
  prof_begin("asm_reduce", s);
  hipLaunchKernelGGL(k_asm_mark, dim3((unsigned)nb_ev), dim3(ASM_WG), 0, s, sort.keys(), (uint32_t)n, (uint32_t)(c.min_cov > 1 ? c.min_cov : 1), flag);
  const int rc_scan = scan_exclusive_u32(flag, out, (int64_t)n, &w.sc->nkept, b->scan_tmp, s);
  prof_end("asm_reduce", s);
  EPI_TRY(rc_scan);
  EPI_HIP(hipGetLastError());
  AsmScalars h;
  EPI_TRY(read_scalars(b, s, w.sc, sizeof(h), &h));
  if (h.overflow || h.cursor != ne)
    return fail(EPI_ERR_STATE, "%s: sites %lld to %lld counted %llu events and wrote %llu", who, (long long)ga, (long long)gb - 1, ne, h.cursor);
  if (h.nkept) EPI_TRY(asm_piece(b, c, w, sort, n, ga, h.nkept, s));
  *npair += h.nkept;
  return EPI_OK;
}

// (g) the SNV rows; the overflow verdict is the last synchronisation
static int asm_snv_rows(epi_batch *b, const AsmCall &c, const AsmWork &w, hipStream_t s) {
  const char *who = "epi_batch_asm_report_dev";
  prof_begin("asm_snv", s);
  hipLaunchKernelGGL(k_asm_snv, dim3((unsigned)((c.nsite + 255) / 256)), dim3(ASM_WG), 0, s, c.d_chr, c.d_pos, c.nsite, w.d_reads, w.d_npairs,
                     w.d_pooled, c.snv, w.sc);
  prof_end("asm_snv", s);
  EPI_HIP(hipGetLastError());
  AsmScalars h;
  EPI_TRY(read_scalars(b, s, w.sc, sizeof(h), &h));
  if (h.bad_sum) return fail(EPI_ERR_ARG, "%s: site %u has a count above 2^31 - 1, which an int32 column cannot hold", who, h.bad_sum - 1u);
  return EPI_OK;
}

static int asm_report(epi_batch *b, const AsmCall &c, hipStream_t s, int64_t *npair_out) {
  const char *who = "epi_batch_asm_report_dev";
  AsmState &st = b->asmr;
  st.clear();
  AsmWork w;
  EPI_TRY(asm_sites(b, c, w, s));
  std::vector<unsigned long long> h_ev;
  EPI_TRY(asm_count(b, c, w, s, h_ev));
  const int64_t cap_bytes = options().asm_group_bytes > 0 ? options().asm_group_bytes : kAsmGroupBytes;
  const int64_t max_sites = 1LL << (58u - w.qbits < 31u ? 58u - w.qbits : 31u);
  int64_t npair = 0;
  for (int64_t ga = 0, gb = 0; ga < (int64_t)h_ev.size(); ga = gb) {
    unsigned long long ne = 0;
    gb = asm_group_end(h_ev, ga, max_sites, cap_bytes, &ne);
    if (ne > 0x7FFFFFFFull)
      return fail(EPI_ERR_ARG, "%s: site %lld has %llu events, a site is sorted with at most 2^31 - 1", who, (long long)ga, ne);
    if (ne > 0) EPI_TRY(asm_group(b, c, w, ga, gb, ne, s, &npair));
  }
  EPI_TRY(asm_snv_rows(b, c, w, s));
  st.npair = npair;
  st.reported = true;
  *npair_out = npair;
  return EPI_OK;
}

}  // namespace epi

using namespace epi;

extern "C" {

int epi_asm_event_bytes(int64_t nevents, int64_t *bytes_out) {
  if (!bytes_out) return fail(EPI_ERR_ARG, "epi_asm_event_bytes: NULL argument");
  *bytes_out = 0;
  const int64_t bytes = asm_event_bytes(nevents);
  if (bytes < 0) return fail(EPI_ERR_ARG, "epi_asm_event_bytes: %lld events, a group of sites holds 0 to 2^32 - 1", (long long)nevents);
  *bytes_out = bytes;
  return EPI_OK;
}

int epi_batch_asm_report_dev(epi_batch *b, const int32_t *d_site_chr, const int32_t *d_site_pos, const int32_t *d_site_alleles,
                             int64_t nsite, const char *ctx, int32_t max_distance, int32_t min_coverage, double max_ooctx_meth_frac,
                             int32_t *const d_snv_icols[10], double *const d_snv_dcols[4], void *stream, int64_t *npair_out) {
  const char *who = "epi_batch_asm_report_dev";
  if (!b) return fail(EPI_ERR_ARG, "%s: batch is NULL", who);
  if (!npair_out) return fail(EPI_ERR_ARG, "%s: npair_out is NULL", who);
  *npair_out = 0;
  if (!ctx) return fail(EPI_ERR_ARG, "%s: ctx is NULL", who);
  if (nsite < 0 || nsite > 0x7FFFFFFFLL) return fail(EPI_ERR_ARG, "%s: nsite = %lld, 0 to 2^31 - 1 sites", who, (long long)nsite);
  if (max_distance < 0) return fail(EPI_ERR_ARG, "%s: max_distance = %d is negative", who, max_distance);
  if (min_coverage < 0) return fail(EPI_ERR_ARG, "%s: min_coverage = %d is negative", who, min_coverage);
  if (nsite > 0) {
    if (!d_site_chr || !d_site_pos || !d_site_alleles) return fail(EPI_ERR_ARG, "%s: d_site_chr, d_site_pos or d_site_alleles is NULL", who);
    if (!d_snv_icols || !d_snv_dcols) return fail(EPI_ERR_ARG, "%s: d_snv_icols or d_snv_dcols is NULL", who);
    for (int i = 0; i < 10; i++) if (!d_snv_icols[i]) return fail(EPI_ERR_ARG, "%s: d_snv_icols[%d] is NULL", who, i);
    for (int i = 0; i < 4; i++) if (!d_snv_dcols[i]) return fail(EPI_ERR_ARG, "%s: d_snv_dcols[%d] is NULL", who, i);
  }
  EPI_HIP(hipSetDevice(b->eng->device));                       // (the last report's table goes: its device must be current)
  if (nsite == 0) {
    b->asmr.clear();
    b->asmr.reported = true;
    return EPI_OK;
  }
  AsmCall c;
  c.d_chr = d_site_chr; c.d_pos = d_site_pos; c.d_all = d_site_alleles; c.nsite = nsite;
  c.ctx = ctx; c.max_dist = max_distance; c.min_cov = min_coverage; c.max_oo = max_ooctx_meth_frac;
  for (int i = 0; i < 10; i++) c.snv.icol[i] = d_snv_icols[i];
  for (int i = 0; i < 4; i++) c.snv.dcol[i] = d_snv_dcols[i];
  const int rc = asm_report(b, c, pick_stream(b, stream), npair_out);
  if (rc != EPI_OK) b->asmr.clear();                           // no table, and no piece of one, outlives a failed report
  return rc;
}

int epi_batch_asm_fetch_dev(epi_batch *b, int32_t *const d_icols[10], double *const d_dcols[4], void *stream) {
  const char *who = "epi_batch_asm_fetch_dev";
  if (!b) return fail(EPI_ERR_ARG, "%s: batch is NULL", who);
  const AsmState &st = b->asmr;
  if (!st.reported) return fail(EPI_ERR_STATE, "%s: no allele-specific methylation report on this batch", who);
  if (st.npair == 0) return EPI_OK;
  if (!d_icols || !d_dcols) return fail(EPI_ERR_ARG, "%s: d_icols or d_dcols is NULL", who);
  AsmCols o;
  for (int i = 0; i < 10; i++) { if (!d_icols[i]) return fail(EPI_ERR_ARG, "%s: d_icols[%d] is NULL", who, i); o.icol[i] = d_icols[i]; }
  for (int i = 0; i < 4; i++) { if (!d_dcols[i]) return fail(EPI_ERR_ARG, "%s: d_dcols[%d] is NULL", who, i); o.dcol[i] = d_dcols[i]; }
  EPI_HIP(hipSetDevice(b->eng->device));
  hipStream_t s = pick_stream(b, stream);
  int64_t row0 = 0;
  prof_begin("asm_fetch", s);
  for (size_t k = 0; k < st.piece.size(); k++) {
    const int64_t nr = st.rows[k], nb = (nr + ASM_WG - 1) / ASM_WG;
    if (nr == 0) continue;
    hipLaunchKernelGGL(k_asm_fetch, dim3((unsigned)nb), dim3(ASM_WG), 0, s, st.piece[k].as<int32_t>(), nr, row0, o);
    row0 += nr;
  }
  prof_end("asm_fetch", s);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

}  // extern "C"
