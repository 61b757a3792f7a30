// rcpp_extract_patterns (src/rcpp_extract_patterns.cpp:26-211): methylation patterns of the reads that overlap one
// target region.  The work is confined to that region (a few thousand reads), so this is three small kernels around
// two host decisions, not a bandwidth problem:
//   k_pat_flag     one thread per row: does the read overlap the target by min_overlap (:79-86)?  -> scan -> its index
//   k_pat_count    one thread per overlapping read: how often is each in-context position seen (:87-96)
//   host           valid positions = seen in >= min_ctx_freq of the overlapping reads and not highlighted (:103-108),
//                  merged with the highlight positions, ordered (:185)
//   k_pat_extract  one thread per overlapping read: its cell per valid position, methylated / total counts and the
//                  FNV-1a hash of (position, base) pairs, highlighted bases appended (:133-166)
//   host           drops empty patterns (:152) and returns the table.
// epi_batch_extract_patterns_multi (second half of this file) runs the same per-read rules for every target of a list in
// O(1) launches and host round trips: candidate row ranges by search, one flat list of (target, row) pairs.
// epi_batch_summarise_patterns_multi runs the same two passes and then groups every target's patterns on the device
// (k_pats_*): only the unique patterns and their counts come to the host.
// Quirks of the reference kept as they are: with clip=TRUE the byte loop ends at `overlap`,
// not at begin+overlap (:86,:132), and position bytes enter the hash sign-extended (char pointer, epialleleR.h:8-13).
#include "common.hpp"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <unordered_map>
#include <vector>

namespace epi {

struct PatArgs {
  const uint8_t *xm;
  const int64_t *off;             // row x owns xm[off[x] .. off[x] + len[x])
  const int32_t *len;
  const int32_t *rname, *strand, *start;
  int64_t n;
  uint32_t target_rname, target_start, target_end, reverse_offset;
  int32_t min_overlap, clip;
  uint32_t ctx_mask;
  int64_t pos_lo;                 // window of positions that can occur: [pos_lo, pos_lo + nwin)
  int64_t nwin;
};

struct PatSpan { uint32_t start_x, begin_i, end_i, offset_x; bool ok; };

__device__ __forceinline__ PatSpan pat_span(const PatArgs &a, int64_t x) {
  PatSpan s;
  s.ok = false; s.start_x = 0; s.begin_i = 0; s.end_i = 0; s.offset_x = 0;
  if (a.rname[x] != (int32_t)a.target_rname) return s;                      // :78
  const uint32_t size_x = (uint32_t)a.len[x];
  const uint32_t start_x = (uint32_t)a.start[x];
  const uint32_t end_x = start_x + size_x - 1u;
  const uint32_t over_start = start_x > a.target_start ? start_x : a.target_start;
  const uint32_t over_end = end_x < a.target_end ? end_x : a.target_end;
  const int32_t overlap = (int32_t)(over_end - over_start + 1u);            // :84
  if (overlap < a.min_overlap) return s;
  s.ok = true;
  s.start_x = start_x;
  s.offset_x = a.strand[x] == 2 ? a.reverse_offset : 0u;
  s.begin_i = a.clip ? over_start - start_x : 0u;
  s.end_i = a.clip ? (uint32_t)overlap : size_x;
  if (s.end_i > size_x) s.end_i = size_x;                                   // (the reference would read past the string)
  return s;
}

__global__ __launch_bounds__(256) void k_pat_flag(PatArgs a, uint32_t *__restrict__ flag) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= a.n) return;
  flag[x] = pat_span(a, x).ok ? 1u : 0u;
}

// row x overlaps the target (s = pat_span(a, x), s.ok): one count per in-context position of its span
__device__ __forceinline__ void pat_count_row(const PatArgs &a, int64_t x, const PatSpan &s, uint32_t *__restrict__ cnt) {
  const uint8_t *p = a.xm + a.off[x];
  for (uint32_t i = s.begin_i; i < s.end_i; i++) {
    if (!((a.ctx_mask >> (p[i] & 15u)) & 1u)) continue;
    const int64_t w = (int64_t)(int32_t)(s.start_x + i - s.offset_x) - a.pos_lo;
    if (w >= 0 && w < a.nwin) atomicAdd(cnt + w, 1u);
  }
}

__global__ __launch_bounds__(256) void k_pat_count(PatArgs a, const uint32_t *__restrict__ flag, uint32_t *__restrict__ cnt) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= a.n || !flag[x]) return;
  pat_count_row(a, x, pat_span(a, x), cnt);
}

struct PatOut {
  int32_t *nonempty, *strand, *start, *end, *nbase, *meth;
  unsigned long long *fnv;
  int32_t *cells;                 // [ncol][npat0]
};

__device__ __forceinline__ void fnv_char(unsigned long long &h, uint32_t v) {   // four bytes through a (signed) char pointer
#pragma unroll
  for (int k = 0; k < 4; k++) {
    h ^= (unsigned long long)(long long)(signed char)((v >> (8 * k)) & 0xFFu);
    h *= 1099511628211ull;
  }
}

// row x overlaps the target (s = pat_span(a, x), s.ok) and is its c-th overlapping row: cells, counts and hash
__device__ __forceinline__ void pat_extract_row(const PatArgs &a, int64_t x, const PatSpan &s, uint32_t c,
                                                const int32_t *__restrict__ colmap, const int32_t *__restrict__ hlght,
                                                const int32_t *__restrict__ hcol, int32_t nhlght, int64_t npat0, const PatOut &o) {
  const uint8_t *p = a.xm + a.off[x];
  uint32_t meth = 0, total = 0;
  unsigned long long fnv = 14695981039346656037ull;
  for (uint32_t i = s.begin_i; i < s.end_i; i++) {
    const uint32_t base = p[i] & 15u;
    if (!((a.ctx_mask >> base) & 1u)) continue;
    const uint32_t pos = s.start_x + i - s.offset_x;
    const int64_t w = (int64_t)(int32_t)pos - a.pos_lo;
    if (w < 0 || w >= a.nwin) continue;
    const int32_t col = colmap[w];
    if (col < 0) continue;                                                   // :141
    o.cells[(int64_t)col * npat0 + c] = (int32_t)base;                       // :143
    meth += !(base & 8u);
    total++;
    fnv_char(fnv, pos);                                                      // :147
    fnv ^= (unsigned long long)base; fnv *= 1099511628211ull;                // :148
  }
  const bool nonempty = fnv != 14695981039346656037ull;
  if (nonempty) {
    static const uint8_t factor_map[16] = {13, 3, 4, 13, 11, 13, 13, 13, 12, 13, 13, 13, 13, 13, 13, 13};   // :47
    for (int32_t k = 0; k < nhlght; k++) {                                   // :154-164
      const uint32_t hp = (uint32_t)hlght[k] - s.start_x;
      if (hp >= s.begin_i && hp < s.end_i) {
        const uint32_t base = factor_map[(p[hp] >> 4) & 15u];
        o.cells[(int64_t)hcol[k] * npat0 + c] = (int32_t)base;
        fnv_char(fnv, (uint32_t)hlght[k]);
        fnv ^= (unsigned long long)base; fnv *= 1099511628211ull;
      }
    }
  }
  o.nonempty[c] = nonempty ? 1 : 0;
  o.strand[c] = a.strand[x];
  o.start[c] = (int32_t)(s.start_x + s.begin_i);
  o.end[c] = (int32_t)(s.start_x + s.end_i - 1u);
  o.nbase[c] = (int32_t)total;
  o.meth[c] = (int32_t)meth;
  o.fnv[c] = fnv;
}

__global__ __launch_bounds__(256) void k_pat_extract(PatArgs a, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ cidx,
                                                      const int32_t *__restrict__ colmap, const int32_t *__restrict__ hlght,
                                                      const int32_t *__restrict__ hcol, int32_t nhlght, int64_t npat0, PatOut o) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= a.n || !flag[x]) return;
  pat_extract_row(a, x, pat_span(a, x), cidx[x], colmap, hlght, hcol, nhlght, npat0, o);
}

// ---- every target of a list at once (epi_batch_extract_patterns_multi) -------------------------------------------------
// Rows sorted by (rname, start): the rows that can overlap target t lie in one range [row_lo, row_hi), found by search.
// The ranges of a group of targets are laid end to end as one flat list of (target, candidate row) pairs; pre[] is the
// u64 exclusive scan of the range lengths, and thread j finds its target as the last t with pre[t] <= j.  flag / cidx
// are indexed by pair, cnt / colmap by the targets' windows laid end to end: every target owns a slice of each.
struct PatTarget {
  int64_t row_lo;                 // its candidate rows: row_lo + (j - pre[t])
  int64_t pos_lo, nwin;           // its window of positions, as PatArgs
  int64_t win_off;                // its slice of cnt / colmap
  int64_t hl_off;                 // its highlight positions: hl[hl_off .. hl_off + nhl), columns hcol[...]
  int32_t rname, start, end, nhl;
};
struct PatSlice {                 // what the host decided for a target between the two passes
  int64_t cell_off;               // its [ncol][npat0] cells in the cell scratch
  uint32_t base_abs;              // cidx of its first overlapping row
  uint32_t base_rel;              // its first slot in the per-pattern arrays
  uint32_t npat0, pad;
};
struct PatMulti {
  const uint8_t *xm;
  const int64_t *off;
  const int32_t *len, *rname, *strand, *start;
  uint32_t reverse_offset, ctx_mask;
  int32_t min_overlap, clip;
  const PatTarget *tg;
  const uint64_t *pre;            // [ng + 1]
  int32_t ng;
};

__device__ __forceinline__ PatArgs pat_args_of(const PatMulti &m, const PatTarget &g) {
  PatArgs a;
  a.xm = m.xm; a.off = m.off; a.len = m.len; a.rname = m.rname; a.strand = m.strand; a.start = m.start; a.n = 0;
  a.target_rname = (uint32_t)g.rname; a.target_start = (uint32_t)g.start; a.target_end = (uint32_t)g.end;
  a.reverse_offset = m.reverse_offset; a.min_overlap = m.min_overlap; a.clip = m.clip; a.ctx_mask = m.ctx_mask;
  a.pos_lo = g.pos_lo; a.nwin = g.nwin;
  return a;
}

// last t in [0, ng) with pre[t] <= j (pre[0] = 0 <= j < pre[ng]); at most 32 steps
__device__ __forceinline__ int32_t pat_target_of(const uint64_t *__restrict__ pre, int32_t ng, uint64_t j) {
  int32_t a = 0, b = ng;
  for (int it = 0; it < 32 && b - a > 1; it++) {
    const int32_t m = a + ((b - a) >> 1);
    if (pre[m] <= j) a = m; else b = m;
  }
  return a;
}

// first row in [0, n) with (rname, start) >= (qr, qp); at most 64 steps
__device__ __forceinline__ int64_t pat_row_lower_bound(const int32_t *__restrict__ rname, const int32_t *__restrict__ start, int64_t n,
                                                       int32_t qr, int64_t qp) {
  int64_t a = 0, b = n;
  for (int it = 0; it < 64 && a < b; it++) {
    const int64_t m = a + ((b - a) >> 1);
    const int32_t r = rname[m];
    if (r < qr || (r == qr && (int64_t)start[m] < qp)) a = m + 1; else b = m;
  }
  return a;
}

// One lane per target: rng[2t], rng[2t+1] = its candidate rows, those on its rname that start in
// [start - reach - lmax + 1, end + reach] (reach = 0 for min_overlap >= 1: pat_span accepts no other row).
// rng[2 * nt] != 0: some target's rname holds a row with a negative start (pat_span's unsigned arithmetic lets such a
// row overlap anything; the caller takes the per-target path).
__global__ __launch_bounds__(256) void k_patm_ranges(const int32_t *__restrict__ rname, const int32_t *__restrict__ start, int64_t n,
                                                     const int32_t *__restrict__ tgt /* [3][nt] rname, start, end */, int32_t nt,
                                                     int64_t lmax, int64_t reach, int64_t *__restrict__ rng) {
  const int32_t t = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (t >= nt) return;
  const int32_t qr = tgt[t];
  const int64_t ts = tgt[nt + t], te = tgt[2 * (int64_t)nt + t];
  const int64_t lo = pat_row_lower_bound(rname, start, n, qr, ts - reach - lmax + 1);
  int64_t hi = pat_row_lower_bound(rname, start, n, qr, te + reach + 1);
  if (hi < lo) hi = lo;
  rng[2 * (int64_t)t] = lo;
  rng[2 * (int64_t)t + 1] = hi;
  const int64_t first = pat_row_lower_bound(rname, start, n, qr, INT64_MIN);
  if (first < n && rname[first] == qr && start[first] < 0) rng[2 * (int64_t)nt] = 1;
}

// pass 1, one thread per pair: does the row overlap its target (-> flag), and if so its in-context positions (-> cnt)
__global__ __launch_bounds__(256) void k_patm_flag_count(PatMulti m, uint64_t npairs, uint32_t *__restrict__ flag, uint32_t *__restrict__ cnt) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= npairs) return;
  const int32_t t = pat_target_of(m.pre, m.ng, j);
  const PatTarget g = m.tg[t];
  const PatArgs a = pat_args_of(m, g);
  const int64_t x = g.row_lo + (int64_t)(j - m.pre[t]);
  const PatSpan s = pat_span(a, x);
  flag[j] = s.ok ? 1u : 0u;
  if (s.ok) pat_count_row(a, x, s, cnt + g.win_off);
}

// base[t] = overlapping rows before target t's range (base[ng], the total, is the scan's)
__global__ __launch_bounds__(256) void k_patm_bases(const uint64_t *__restrict__ pre, int32_t ng, uint64_t npairs,
                                                    const uint32_t *__restrict__ cidx, uint32_t *__restrict__ base) {
  const int32_t t = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (t >= ng) return;
  base[t] = pre[t] < npairs ? cidx[pre[t]] : base[ng];
}

// pass 2, one thread per pair j0 + k, k < npairs: the pairs of the group's targets whose results share the scratch this time
__global__ __launch_bounds__(256) void k_patm_extract(PatMulti m, uint64_t j0, uint64_t npairs, const uint32_t *__restrict__ flag,
                                                      const uint32_t *__restrict__ cidx, const PatSlice *__restrict__ sl,
                                                      const int32_t *__restrict__ colmap, const int32_t *__restrict__ hl,
                                                      const int32_t *__restrict__ hcol, PatOut o) {
  const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= npairs) return;
  const uint64_t j = j0 + k;
  if (!flag[j]) return;
  const int32_t t = pat_target_of(m.pre, m.ng, j);
  const PatTarget g = m.tg[t];
  const PatSlice q = sl[t];
  const PatArgs a = pat_args_of(m, g);
  const int64_t x = g.row_lo + (int64_t)(j - m.pre[t]);
  PatOut ot;
  ot.nonempty = o.nonempty + q.base_rel; ot.strand = o.strand + q.base_rel; ot.start = o.start + q.base_rel; ot.end = o.end + q.base_rel;
  ot.nbase = o.nbase + q.base_rel; ot.meth = o.meth + q.base_rel; ot.fnv = o.fnv + q.base_rel;
  ot.cells = o.cells + q.cell_off;
  pat_extract_row(a, x, pat_span(a, x), cidx[j] - q.base_abs, colmap + g.win_off, hl + g.hl_off, hcol + g.hl_off, g.nhl, (int64_t)q.npat0, ot);
}

// ---- unique patterns with their counts (epi_batch_summarise_patterns_multi) --------------------------------------------
// R/plotPatterns.R:172, patterns[, .(count=.N), by=c("pattern", base.positions)], for every target of a cell batch while its
// slots (fnv, nonempty, cells[ncol][npat0]) are on the device.  Every target owns a slice of one open-addressing table
// (power-of-two capacity >= 2 x its slots, keyed by the hash; the FNV offset basis, which no non-empty pattern has, is the
// empty key).  insert -> verify (a slot whose cells differ from those of its entry's first slot: two patterns share a key,
// the target is flagged and the host groups it by (hash, cells) instead) -> scans of the first-occurrence flags -> emit.
struct PatEntry { unsigned long long key; uint32_t count, first; };
struct PatSumSlice {              // a target's slice of the table
  int64_t tab_off;
  uint32_t mask;                  // capacity - 1
  uint32_t ncol;
};
struct PatSum {
  const PatSlice *sl;             // the group's targets; this batch: [sa, sb), slots [0, nslot) by base_rel
  const PatSumSlice *ss;
  int32_t sa, sb;
  uint32_t nslot;
  const unsigned long long *fnv;
  const int32_t *nonempty, *cells;
  PatEntry *tab;
  uint32_t *ent;                  // [nslot] a slot's entry inside its target's slice
  uint32_t *collide;              // [sb - sa]
  unsigned long long key_mask;    // EPIHIP_PAT_HASH_BITS
};
constexpr unsigned long long kPatEmptyKey = 14695981039346656037ull;

// last t in [sa, sb) with sl[t].base_rel <= i (targets without slots share their successor's base_rel and come before it)
__device__ __forceinline__ int32_t pat_slot_target(const PatSlice *__restrict__ sl, int32_t sa, int32_t sb, uint32_t i) {
  int32_t a = sa, b = sb;
  for (int it = 0; it < 32 && b - a > 1; it++) {
    const int32_t m = a + ((b - a) >> 1);
    if (sl[m].base_rel <= i) a = m; else b = m;
  }
  return a;
}

__global__ __launch_bounds__(256) void k_pats_init(PatEntry *__restrict__ tab, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  PatEntry v;
  v.key = kPatEmptyKey; v.count = 0u; v.first = 0xFFFFFFFFu;
  tab[e] = v;
}

// the entry of `key` in the slice s: linear probe from the key's home, the slice is never full (capacity >= 2 x slots)
__device__ __forceinline__ bool pat_probe(PatEntry *__restrict__ e0, uint32_t mask, unsigned long long key, uint32_t &p) {
  p = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
  for (uint32_t step = 0; step <= mask; step++) {
    const unsigned long long prev = atomicCAS(&e0[p].key, kPatEmptyKey, key);
    if (prev == kPatEmptyKey || prev == key) return true;
    p = (p + 1u) & mask;
  }
  return false;
}

// One thread per slot.  A deep amplicon has most of its reads on one pattern, so a wave adds once per distinct
// (target, key) among its lanes, not once per lane: the lowest remaining lane's pair is broadcast, the lanes that hold
// the same pair are balloted, and that lane (the leader; slots rise with the lane, so its slot is the smallest of them)
// probes and adds the ballot's population count.  EPI_PATS_PER_LANE (timing builds): every lane probes and adds 1.
__global__ __launch_bounds__(256) void k_pats_insert(PatSum q) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool todo = i < q.nslot && q.nonempty[i] != 0;
  int32_t t = 0;
  unsigned long long key = 0;
  if (todo) {
    t = pat_slot_target(q.sl, q.sa, q.sb, i);
    key = q.fnv[i] & q.key_mask;
  }
  const bool mine = todo;
  uint32_t e = 0;
#ifdef EPI_PATS_PER_LANE
  if (todo) {
    const PatSumSlice s = q.ss[t];
    PatEntry *e0 = q.tab + s.tab_off;
    if (pat_probe(e0, s.mask, key, e)) { atomicAdd(&e0[e].count, 1u); atomicMin(&e0[e].first, i); }
    else q.collide[t - q.sa] = 1u;
  }
#else
  while (todo) {
    const int32_t t0 = __builtin_amdgcn_readfirstlane(t);
    const uint32_t lo0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)key);
    const uint32_t hi0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(key >> 32));
    const bool match = t == t0 && (uint32_t)key == lo0 && (uint32_t)(key >> 32) == hi0;
    const unsigned long long mb = __ballot(match);
    uint32_t p = 0;
    if ((uint32_t)(__ffsll((long long)mb) - 1) == (threadIdx.x & 63u)) {    // the leader: the lowest lane still here
      const PatSumSlice s = q.ss[t];
      PatEntry *e0 = q.tab + s.tab_off;
      if (pat_probe(e0, s.mask, key, p)) { atomicAdd(&e0[p].count, (uint32_t)__popcll(mb)); atomicMin(&e0[p].first, i); }
      else q.collide[t - q.sa] = 1u;
    }
    p = (uint32_t)__builtin_amdgcn_readfirstlane((int)p);
    if (match) { e = p; todo = false; }
  }
#endif
  if (mine) q.ent[i] = e;
}

// first[i] = 1 for a slot that is the first of its entry (wfirst: its ncol, the cells it will emit); every other
// non-empty slot compares its hash and cells with that first slot's, column by column (neighbouring slots coalesce)
__global__ __launch_bounds__(256) void k_pats_verify(PatSum q, uint32_t *__restrict__ first, uint32_t *__restrict__ wfirst) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= q.nslot) return;
  uint32_t f1 = 0, w = 0;
  if (q.nonempty[i]) {
    const int32_t t = pat_slot_target(q.sl, q.sa, q.sb, i);
    const PatSlice sl = q.sl[t];
    const PatSumSlice ss = q.ss[t];
    const uint32_t f = q.tab[ss.tab_off + (q.ent[i] & ss.mask)].first;
    if (f == i) {
      f1 = 1u; w = ss.ncol;
    } else if (f < sl.base_rel || f > i) {                             // (only after a failed probe)
      q.collide[t - q.sa] = 1u;
    } else {
      bool same = q.fnv[i] == q.fnv[f];
      const int32_t *c = q.cells + sl.cell_off;
      const uint32_t li = i - sl.base_rel, lf = f - sl.base_rel;
      for (uint32_t k = 0; k < ss.ncol; k++) same = same && c[(int64_t)k * sl.npat0 + li] == c[(int64_t)k * sl.npat0 + lf];
      if (!same) q.collide[t - q.sa] = 1u;
    }
  }
  first[i] = f1;
  wfirst[i] = w;
}

// ubase[k] / wbase[k] = unique patterns / emitted cells before the batch's k-th target (the totals, [nb], are the scans')
__global__ __launch_bounds__(256) void k_pats_bases(const PatSlice *__restrict__ sl, int32_t sa, int32_t nb, uint32_t nslot,
                                                    const uint32_t *__restrict__ uidx, const uint32_t *__restrict__ widx,
                                                    uint32_t *__restrict__ ubase, uint32_t *__restrict__ wbase) {
  const int32_t k = (int32_t)(blockIdx.x * 256 + threadIdx.x);
  if (k >= nb) return;
  const uint32_t r = sl[sa + k].base_rel;
  ubase[k] = r < nslot ? uidx[r] : ubase[nb];
  wbase[k] = r < nslot ? widx[r] : wbase[nb];
}

// out: [fnv u64 x U][count u32 x U][cells i32, per target [ncol][nuniq]], U = ubase[nb] <= nslot
__global__ __launch_bounds__(256) void k_pats_emit(PatSum q, const uint32_t *__restrict__ first, const uint32_t *__restrict__ uidx,
                                                   const uint32_t *__restrict__ ubase, const uint32_t *__restrict__ wbase,
                                                   unsigned long long *__restrict__ out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= q.nslot || !first[i]) return;
  const int32_t t = pat_slot_target(q.sl, q.sa, q.sb, i);
  const int32_t k = t - q.sa, nb = q.sb - q.sa;
  const PatSlice sl = q.sl[t];
  const PatSumSlice ss = q.ss[t];
  const uint32_t U = ubase[nb], u = uidx[i], nu = ubase[k + 1] - ubase[k], lu = u - ubase[k], li = i - sl.base_rel;
  uint32_t *count = reinterpret_cast<uint32_t *>(out + U);
  int32_t *oc = reinterpret_cast<int32_t *>(count + U) + wbase[k];
  out[u] = q.fnv[i];
  count[u] = q.tab[ss.tab_off + (q.ent[i] & ss.mask)].count;
  const int32_t *c = q.cells + sl.cell_off;
  for (uint32_t col = 0; col < ss.ncol; col++) oc[(int64_t)col * nu + lu] = c[(int64_t)col * sl.npat0 + li];
}

}  // namespace epi

using namespace epi;

extern "C" void epi_pattern_table_free(epi_pattern_table *t);
extern "C" void epi_pattern_summary_free(epi_pattern_summary *t);

// The host's decision between the two passes: valid positions = seen in >= min_ctx_freq of the npat0 overlapping reads
// and not highlighted (:103-108), the highlight positions (:110-112), merged in position order (:185).  cnt / colmap:
// the nwin positions from pos_lo on (colmap: column of a valid position, else -1); hcol[k]: column of hlght[k].
static void pat_choose_columns(const uint32_t *cnt, int64_t nwin, int64_t pos_lo, uint32_t npat0, double min_ctx_freq,
                               const int32_t *hlght, int32_t nhlght, std::vector<int32_t> &cols, int32_t *colmap, int32_t *hcol) {
  cols.clear();
  for (int64_t w = 0; w < nwin; w++) {
    colmap[w] = -1;
    if (!cnt[w]) continue;
    const int32_t pos = (int32_t)(pos_lo + w);
    if ((double)cnt[w] / npat0 >= min_ctx_freq && std::find(hlght, hlght + nhlght, pos) == hlght + nhlght) cols.push_back(pos);
  }
  const size_t npatcols = cols.size();
  for (int32_t k = 0; k < nhlght; k++) cols.push_back(hlght[k]);
  std::vector<int32_t> patcols(cols.begin(), cols.begin() + (long)npatcols);
  std::sort(cols.begin(), cols.end());
  cols.erase(std::unique(cols.begin(), cols.end()), cols.end());       // std::map keys are unique
  for (int32_t pos : patcols) colmap[(int64_t)pos - pos_lo] = (int32_t)(std::lower_bound(cols.begin(), cols.end(), pos) - cols.begin());
  for (int32_t k = 0; k < nhlght; k++) hcol[k] = (int32_t)(std::lower_bound(cols.begin(), cols.end(), hlght[k]) - cols.begin());
}

// The table of one target from the P0 slots its overlapping rows filled: keeps the non-empty patterns, in row order
// (:152, :166-176).  cells: [ncol][P0].
static int pat_fill_table(epi_pattern_table *out, size_t P0, int32_t ncol, const int32_t *cols, const int32_t *nonempty,
                          const int32_t *strand, const int32_t *start, const int32_t *end, const int32_t *nbase, const int32_t *meth,
                          const unsigned long long *fnv, const int32_t *cells) {
  size_t np = 0;
  for (size_t c = 0; c < P0; c++) np += nonempty[c] != 0;
  if (np == 0) return EPI_OK;
  out->npat = (int64_t)np;
  out->ncol = ncol;
  out->positions = (int32_t *)malloc(((size_t)ncol + 1) * 4);
  out->strand = (int32_t *)malloc(np * 4); out->start = (int32_t *)malloc(np * 4); out->end = (int32_t *)malloc(np * 4);
  out->nbase = (int32_t *)malloc(np * 4); out->beta = (double *)malloc(np * 8); out->fnv = (uint64_t *)malloc(np * 8);
  out->cells = (int32_t *)malloc(((size_t)ncol * np + 1) * 4);
  if (!out->positions || !out->strand || !out->start || !out->end || !out->nbase || !out->beta || !out->fnv || !out->cells) {
    epi_pattern_table_free(out);
    return fail(EPI_ERR_NOMEM, "epi_batch_extract_patterns: out of host memory");
  }
  memcpy(out->positions, cols, (size_t)ncol * 4);
  size_t w = 0;
  for (size_t c = 0; c < P0; c++) {
    if (!nonempty[c]) continue;
    out->strand[w] = strand[c]; out->start[w] = start[c]; out->end[w] = end[c];
    out->nbase[w] = nbase[c];
    out->beta[w] = (double)(uint32_t)meth[c] / (uint32_t)nbase[c];                                // :173
    out->fnv[w] = fnv[c];
    for (int32_t k = 0; k < ncol; k++) out->cells[(size_t)k * np + w] = cells[(size_t)k * P0 + c];
    w++;
  }
  return EPI_OK;
}

extern "C" {

void epi_pattern_table_free(epi_pattern_table *t) {
  if (!t) return;
  free(t->positions); free(t->strand); free(t->start); free(t->end); free(t->nbase); free(t->beta); free(t->fnv); free(t->cells);
  memset(t, 0, sizeof(*t));
}

int epi_batch_extract_patterns(epi_batch *b, int32_t target_rname, int32_t target_start, int32_t target_end, int32_t min_overlap,
                               const char *ctx, double min_ctx_freq, int32_t clip, int32_t reverse_offset, const int32_t *hlght,
                               int32_t nhlght, void *stream, epi_pattern_table *out) {
  if (!b || !ctx || !out || nhlght < 0 || (nhlght > 0 && !hlght)) return fail(EPI_ERR_ARG, "epi_batch_extract_patterns: bad arguments");
  memset(out, 0, sizeof(*out));
  if (b->n == 0) return EPI_OK;
  EPI_HIP(hipSetDevice(b->eng->device));
  hipStream_t s = pick_stream(b, stream);
  EPI_TRY(fetch_row_stats(b, s));                           // the longest read bounds the window of positions
  if (b->h_stats.bad_len) return fail(EPI_ERR_ARG, "offsets are not non-decreasing, or start+length exceeds int32");
  const int64_t lmax = b->h_stats.max_len;

  PatArgs a;
  a.xm = b->xm; a.off = b->off; a.len = b->len; a.rname = b->rname; a.strand = b->strand; a.start = b->start; a.n = b->n;
  a.target_rname = (uint32_t)target_rname; a.target_start = (uint32_t)target_start; a.target_end = (uint32_t)target_end;
  a.reverse_offset = (uint32_t)reverse_offset; a.min_overlap = min_overlap; a.clip = clip ? 1 : 0;
  a.ctx_mask = 0;
  for (const unsigned char *c = reinterpret_cast<const unsigned char *>(ctx); *c; c++) a.ctx_mask |= 1u << ctx_to_idx(*c);
  a.pos_lo = (int64_t)target_start - lmax - (int64_t)reverse_offset - 2;
  a.nwin = ((int64_t)target_end - (int64_t)target_start) + 2 * lmax + (int64_t)reverse_offset + 8;
  if (a.nwin < 1) a.nwin = 1;
  if (a.nwin > (1LL << 31)) return fail(EPI_ERR_ARG, "epi_batch_extract_patterns: target too wide");

  const unsigned nb = (unsigned)((b->n + 255) / 256);
  DevBuf flag, cidx, cnt, colmap, d_hl, d_hc, outbuf, cells;
  auto cleanup = [&]() { flag.release(); cidx.release(); cnt.release(); colmap.release(); d_hl.release(); d_hc.release(); outbuf.release(); cells.release(); };
#define PAT_TRY(x) do { int rc_ = (x); if (rc_ != EPI_OK) { cleanup(); return rc_; } } while (0)
#define PAT_HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { cleanup(); return fail(EPI_ERR_HIP, "%s: %s", #x, hipGetErrorString(e_)); } } while (0)
  PAT_TRY(flag.ensure((size_t)b->n * 4));
  PAT_TRY(cidx.ensure((size_t)b->n * 4));
  PAT_TRY(cnt.ensure((size_t)a.nwin * 4));
  PAT_TRY(colmap.ensure((size_t)a.nwin * 4));
  PAT_TRY(b->misc.ensure(256));
  uint32_t *d_total = &report_scalars(b)->pat_total;
  hipLaunchKernelGGL(k_pat_flag, dim3(nb), dim3(256), 0, s, a, flag.as<uint32_t>());
  PAT_TRY(scan_exclusive_u32(flag.as<uint32_t>(), cidx.as<uint32_t>(), b->n, d_total, b->scan_tmp, s));
  PAT_HIP(hipMemsetAsync(cnt.p, 0, (size_t)a.nwin * 4, s));
  hipLaunchKernelGGL(k_pat_count, dim3(nb), dim3(256), 0, s, a, flag.as<uint32_t>(), cnt.as<uint32_t>());
  PAT_HIP(hipGetLastError());
  uint32_t npat0 = 0;
  PAT_TRY(read_scalars(b, s, d_total, 4, &npat0));
  if (npat0 == 0) { cleanup(); return EPI_OK; }             // no read overlaps the target: empty table (:183)
  std::vector<uint32_t> h_cnt((size_t)a.nwin);
  PAT_HIP(hipMemcpy(h_cnt.data(), cnt.p, (size_t)a.nwin * 4, hipMemcpyDeviceToHost));

  std::vector<int32_t> cols;
  std::vector<int32_t> h_colmap((size_t)a.nwin), h_hcol((size_t)(nhlght > 0 ? nhlght : 1), 0);
  pat_choose_columns(h_cnt.data(), a.nwin, a.pos_lo, npat0, min_ctx_freq, hlght, nhlght, cols, h_colmap.data(), h_hcol.data());
  const int32_t ncol = (int32_t)cols.size();
  PAT_HIP(hipMemcpy(colmap.p, h_colmap.data(), (size_t)a.nwin * 4, hipMemcpyHostToDevice));
  PAT_TRY(d_hl.ensure((size_t)(nhlght > 0 ? nhlght : 1) * 4));
  PAT_TRY(d_hc.ensure((size_t)(nhlght > 0 ? nhlght : 1) * 4));
  if (nhlght > 0) {
    PAT_HIP(hipMemcpy(d_hl.p, hlght, (size_t)nhlght * 4, hipMemcpyHostToDevice));
    PAT_HIP(hipMemcpy(d_hc.p, h_hcol.data(), (size_t)nhlght * 4, hipMemcpyHostToDevice));
  }
  const size_t P0 = npat0;
  PAT_TRY(outbuf.ensure(P0 * (6 * 4 + 8) + 64));
  PAT_TRY(cells.ensure((size_t)(ncol > 0 ? ncol : 1) * P0 * 4));
  PatOut o;
  int32_t *ip = outbuf.as<int32_t>();
  o.fnv = reinterpret_cast<unsigned long long *>(ip);                  // 8-byte aligned first
  int32_t *q = ip + 2 * P0;
  o.nonempty = q; o.strand = q + P0; o.start = q + 2 * P0; o.end = q + 3 * P0; o.nbase = q + 4 * P0; o.meth = q + 5 * P0;
  o.cells = cells.as<int32_t>();
  PAT_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(cells.p), INT32_MIN, (size_t)(ncol > 0 ? ncol : 1) * P0, s));   // NA_INTEGER
  hipLaunchKernelGGL(k_pat_extract, dim3(nb), dim3(256), 0, s, a, flag.as<uint32_t>(), cidx.as<uint32_t>(), colmap.as<int32_t>(),
                     d_hl.as<int32_t>(), d_hc.as<int32_t>(), nhlght, (int64_t)P0, o);
  PAT_HIP(hipGetLastError());
  PAT_HIP(hipStreamSynchronize(s));
  std::vector<int32_t> h_i(6 * P0), h_cells((size_t)(ncol > 0 ? ncol : 1) * P0);
  std::vector<unsigned long long> h_f(P0);
  PAT_HIP(hipMemcpy(h_f.data(), o.fnv, P0 * 8, hipMemcpyDeviceToHost));
  PAT_HIP(hipMemcpy(h_i.data(), o.nonempty, 6 * P0 * 4, hipMemcpyDeviceToHost));
  PAT_HIP(hipMemcpy(h_cells.data(), cells.p, h_cells.size() * 4, hipMemcpyDeviceToHost));
  cleanup();
#undef PAT_TRY
#undef PAT_HIP

  const int32_t *r = h_i.data();
  return pat_fill_table(out, P0, ncol, cols.data(), r, r + P0, r + 2 * P0, r + 3 * P0, r + 4 * P0, r + 5 * P0, h_f.data(), h_cells.data());
}

}  // extern "C"

// ---- epi_batch_extract_patterns_multi ---------------------------------------------------------------------------------
namespace {

constexpr int64_t kPatGroupBytes = 256LL << 20;   // scratch cap of a group of targets (include/epihip.h)

struct PatmScratch {
  DevBuf tgt, rng, meta, flag, cidx, cb, colmap, sl, hl, res;
  DevBuf ss, tab, slot, ub, sout;   // the summary path: table slices, table, 5 x u32 per slot, bases and collide words, output
  size_t peak = 0;
  void note() {
    const size_t v = tgt.cap + rng.cap + meta.cap + flag.cap + cidx.cap + cb.cap + colmap.cap + sl.cap + hl.cap + res.cap +
                     ss.cap + tab.cap + slot.cap + ub.cap + sout.cap;
    if (v > peak) peak = v;
  }
  ~PatmScratch() {
    tgt.release(); rng.release(); meta.release(); flag.release(); cidx.release(); cb.release(); colmap.release(); sl.release(); hl.release(); res.release();
    ss.release(); tab.release(); slot.release(); ub.release(); sout.release();
  }
};

struct PatmStats { int64_t groups = 0, pairs = 0, scratch = 0, fallback = 0; };

struct PatmCall {                 // what every group of a call shares
  epi_batch *b;
  hipStream_t s;
  const int32_t *t_rname, *t_start, *t_end;
  const int64_t *row_lo, *row_hi; // [ntargets]
  const int64_t *pos_lo, *nwin;   // [ntargets]
  const int32_t *hlght;
  const int64_t *hlght_off;       // may be null
  double min_ctx_freq;
  int64_t cap;
  PatMulti m;                     // tg / pre / ng filled per group
  epi_pattern_table *out;         // the tables, or ...
  epi_pattern_summary *sum;       // ... the summaries (exactly one of the two is set)
  unsigned long long key_mask;    // the bits of the hash the summary groups by (EPIHIP_PAT_HASH_BITS)
  PatmStats *st;
};

// capacity of a target's table slice: the power of two >= 2 x its slots, 8 at the least (no slots: no slice)
int64_t pat_table_capacity(uint32_t npat0) {
  if (!npat0) return 0;
  int64_t cap = 8;
  while (cap < 2 * (int64_t)npat0) cap <<= 1;
  return cap;
}

// a summary from nuniq unique rows: fnv / count [nuniq], cells [ncol][nuniq]
int pat_fill_summary(epi_pattern_summary *out, size_t nuniq, int32_t ncol, const int32_t *cols, const uint64_t *fnv, const int32_t *count,
                     const int32_t *cells) {
  if (nuniq == 0) return EPI_OK;
  out->nuniq = (int64_t)nuniq;
  out->ncol = ncol;
  out->positions = (int32_t *)malloc(((size_t)ncol + 1) * 4);
  out->fnv = (uint64_t *)malloc(nuniq * 8);
  out->count = (int32_t *)malloc(nuniq * 4);
  out->cells = (int32_t *)malloc(((size_t)ncol * nuniq + 1) * 4);
  if (!out->positions || !out->fnv || !out->count || !out->cells) {
    epi_pattern_summary_free(out);
    return fail(EPI_ERR_NOMEM, "epi_batch_summarise_patterns_multi: out of host memory");
  }
  memcpy(out->positions, cols, (size_t)ncol * 4);
  memcpy(out->fnv, fnv, nuniq * 8);
  memcpy(out->count, count, nuniq * 4);
  memcpy(out->cells, cells, (size_t)ncol * nuniq * 4);
  int64_t np = 0;
  for (size_t u = 0; u < nuniq; u++) np += count[u];
  out->npat = np;
  return EPI_OK;
}

// The host's grouping, by (hash, cells) in order of first appearance: the P0 slots of a target (nonempty: null = all are;
// cells [ncol][P0]).  Exact whatever the hashes are: the summary of a target whose table saw two patterns under one key,
// and of the targets of the target-by-target path.
int pat_summarise_host(epi_pattern_summary *out, size_t P0, int32_t ncol, const int32_t *cols, const int32_t *nonempty,
                       const uint64_t *fnv, const int32_t *cells) {
  std::unordered_multimap<uint64_t, uint32_t> seen;           // hash -> unique rows that have it
  std::vector<uint32_t> first;                                // unique row -> its first slot
  std::vector<int32_t> count;
  for (size_t c = 0; c < P0; c++) {
    if (nonempty && !nonempty[c]) continue;
    auto rng = seen.equal_range(fnv[c]);
    bool found = false;
    for (auto it = rng.first; it != rng.second && !found; ++it) {
      const size_t f = first[it->second];
      bool same = true;
      for (int32_t k = 0; k < ncol && same; k++) same = cells[(size_t)k * P0 + c] == cells[(size_t)k * P0 + f];
      if (same) { count[it->second]++; found = true; }
    }
    if (!found) { seen.emplace(fnv[c], (uint32_t)first.size()); first.push_back((uint32_t)c); count.push_back(1); }
  }
  const size_t U = first.size();
  std::vector<uint64_t> ufnv(U);
  std::vector<int32_t> ucells((size_t)ncol * U + 1);
  for (size_t u = 0; u < U; u++) {
    ufnv[u] = fnv[first[u]];
    for (int32_t k = 0; k < ncol; k++) ucells[(size_t)k * U + u] = cells[(size_t)k * P0 + first[u]];
  }
  return pat_fill_summary(out, U, ncol, cols, ufnv.data(), count.data(), ucells.data());
}

// The summaries of the group's targets [sa, sb), whose Ps slots and C cells pass 2 has just left in `o`: table, verify,
// scans and emit on the device, then two host synchronisations (the unique counts and collide words; the unique rows) and a
// third when targets are regrouped on the host (their slots).
int patm_summarise_batch(PatmCall &c, PatmScratch &w, const std::vector<PatSlice> &sl, const std::vector<PatSumSlice> &ss,
                         const std::vector<std::vector<int32_t>> &cols, int32_t ta, int32_t sa, int32_t sb, size_t Ps, size_t C,
                         const PatOut &o) {
  hipStream_t s = c.s;
  const int32_t nb = sb - sa;
  int64_t TE = 0;
  for (int32_t k = sa; k < sb; k++) TE += pat_table_capacity(sl[(size_t)k].npat0);
  const bool on_device = Ps < (1u << 30) && C < (1u << 31) && TE < (1LL << 32);    // u32 slot and cell indices
  std::vector<uint32_t> h_ub(3 * (size_t)nb + 2, 0);          // ubase[nb + 1], wbase[nb + 1], collide[nb]
  std::vector<uint64_t> h_out;
  if (on_device) {
    const int64_t nbs = (int64_t)((Ps + 255) / 256), nbt = (TE + 255) / 256;
    EPI_TRY(check_grid(nbs, 256, "epi_batch_summarise_patterns_multi"));
    EPI_TRY(check_grid(nbt, 256, "epi_batch_summarise_patterns_multi"));
    EPI_TRY(w.tab.ensure((size_t)TE * sizeof(PatEntry)));
    EPI_TRY(w.slot.ensure(5 * Ps * 4));
    EPI_TRY(w.ub.ensure(h_ub.size() * 4));
    EPI_TRY(w.sout.ensure(12 * Ps + 4 * C + 16));
    w.note();
    uint32_t *ent = w.slot.as<uint32_t>(), *first = ent + Ps, *wfirst = ent + 2 * Ps, *uidx = ent + 3 * Ps, *widx = ent + 4 * Ps;
    uint32_t *ubase = w.ub.as<uint32_t>(), *wbase = ubase + nb + 1, *collide = wbase + nb + 1;
    PatSum q;
    q.sl = w.sl.as<PatSlice>(); q.ss = w.ss.as<PatSumSlice>(); q.sa = sa; q.sb = sb; q.nslot = (uint32_t)Ps;
    q.fnv = o.fnv; q.nonempty = o.nonempty; q.cells = o.cells;
    q.tab = w.tab.as<PatEntry>(); q.ent = ent; q.collide = collide; q.key_mask = c.key_mask;
    EPI_HIP(hipMemsetAsync(w.ub.p, 0, h_ub.size() * 4, s));
    prof_begin("summarise_patterns", s);
    hipLaunchKernelGGL(k_pats_init, dim3((unsigned)nbt), dim3(256), 0, s, q.tab, TE);
    prof_begin("summarise_patterns_insert", s);
    hipLaunchKernelGGL(k_pats_insert, dim3((unsigned)nbs), dim3(256), 0, s, q);
    prof_end("summarise_patterns_insert", s);
    hipLaunchKernelGGL(k_pats_verify, dim3((unsigned)nbs), dim3(256), 0, s, q, first, wfirst);
    EPI_TRY(scan_exclusive_u32(first, uidx, (int64_t)Ps, ubase + nb, c.b->scan_tmp, s));
    EPI_TRY(scan_exclusive_u32(wfirst, widx, (int64_t)Ps, wbase + nb, c.b->scan_tmp, s));
    hipLaunchKernelGGL(k_pats_bases, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, q.sl, sa, nb, q.nslot, uidx, widx, ubase, wbase);
    hipLaunchKernelGGL(k_pats_emit, dim3((unsigned)nbs), dim3(256), 0, s, q, first, uidx, ubase, wbase, w.sout.as<unsigned long long>());
    EPI_HIP(hipGetLastError());
    prof_end("summarise_patterns", s);
    EPI_HIP(hipMemcpyAsync(h_ub.data(), w.ub.p, h_ub.size() * 4, hipMemcpyDeviceToHost, s));
    EPI_HIP(hipStreamSynchronize(s));
    const size_t U = h_ub[(size_t)nb], WC = h_ub[2 * (size_t)nb + 1];
    if (U > Ps || WC > C) return fail(EPI_ERR_STATE, "epi_batch_summarise_patterns_multi: more unique rows than slots");
    h_out.resize((12 * U + 4 * WC + 7) / 8 + 1);
    if (U) {
      EPI_HIP(hipMemcpyAsync(h_out.data(), w.sout.p, 12 * U + 4 * WC, hipMemcpyDeviceToHost, s));
      EPI_HIP(hipStreamSynchronize(s));
    }
  } else {
    EPI_HIP(hipStreamSynchronize(s));
  }
  const uint32_t *ubase = h_ub.data(), *wbase = ubase + nb + 1, *collide = wbase + nb + 1;
  const size_t U = ubase[nb];
  const uint64_t *u_fnv = h_out.data();
  const int32_t *u_count = reinterpret_cast<const int32_t *>(h_out.data() + U), *u_cells = u_count + U;
  struct Slots { int32_t k; std::vector<uint64_t> fnv; std::vector<int32_t> nonempty, cells; };
  std::vector<Slots> back;                                    // the targets the host groups after all, their slots fetched
  for (int32_t k = sa; k < sb; k++) {
    const PatSlice &q1 = sl[(size_t)k];
    if (!q1.npat0) continue;
    const std::vector<int32_t> &ck = cols[(size_t)k];
    const int32_t ncol = (int32_t)ck.size();
    if (on_device && !collide[k - sa]) {
      EPI_TRY(pat_fill_summary(c.sum + ta + k, ubase[k - sa + 1] - ubase[k - sa], ncol, ck.data(), u_fnv + ubase[k - sa],
                               u_count + ubase[k - sa], u_cells + wbase[k - sa]));
      continue;
    }
    // two patterns of this target share a key (or the batch is too large for the device's indices)
    c.st->fallback++;
    const size_t n0 = q1.npat0;
    back.emplace_back();
    Slots &f = back.back();
    f.k = k; f.fnv.resize(n0); f.nonempty.resize(n0); f.cells.resize((size_t)ncol * n0 + 1);
    EPI_HIP(hipMemcpyAsync(f.fnv.data(), o.fnv + q1.base_rel, n0 * 8, hipMemcpyDeviceToHost, s));
    EPI_HIP(hipMemcpyAsync(f.nonempty.data(), o.nonempty + q1.base_rel, n0 * 4, hipMemcpyDeviceToHost, s));
    if (ncol) EPI_HIP(hipMemcpyAsync(f.cells.data(), o.cells + q1.cell_off, (size_t)ncol * n0 * 4, hipMemcpyDeviceToHost, s));
  }
  if (!back.empty()) EPI_HIP(hipStreamSynchronize(s));
  for (const Slots &f : back) {
    const std::vector<int32_t> &ck = cols[(size_t)f.k];
    EPI_TRY(pat_summarise_host(c.sum + ta + f.k, sl[(size_t)f.k].npat0, (int32_t)ck.size(), ck.data(), f.nonempty.data(), f.fnv.data(),
                               f.cells.data()));
  }
  return EPI_OK;
}

// targets [ta, tb): two passes, three host synchronisations (plus one per further cell batch; the summaries: two per cell batch)
int patm_group(PatmCall &c, PatmScratch &w, int32_t ta, int32_t tb) {
  epi_batch *b = c.b;
  hipStream_t s = c.s;
  const int32_t ng = tb - ta;
  std::vector<uint64_t> meta((size_t)(ng + 1) + ((size_t)ng * sizeof(PatTarget) + 7) / 8);
  uint64_t *pre = meta.data();
  PatTarget *tg = reinterpret_cast<PatTarget *>(meta.data() + ng + 1);
  const int64_t hl0 = c.hlght_off ? c.hlght_off[ta] : 0;
  int64_t W = 0;
  pre[0] = 0;
  for (int32_t k = 0; k < ng; k++) {
    const int32_t t = ta + k;
    PatTarget &g = tg[k];
    g.row_lo = c.row_lo[t]; g.pos_lo = c.pos_lo[t]; g.nwin = c.nwin[t]; g.win_off = W;
    g.hl_off = c.hlght_off ? c.hlght_off[t] - hl0 : 0;
    g.nhl = c.hlght_off ? (int32_t)(c.hlght_off[t + 1] - c.hlght_off[t]) : 0;
    g.rname = c.t_rname[t]; g.start = c.t_start[t]; g.end = c.t_end[t];
    W += g.nwin;
    pre[k + 1] = pre[k] + (uint64_t)(c.row_hi[t] - c.row_lo[t]);
  }
  const uint64_t P = pre[ng];
  const int64_t H = c.hlght_off ? c.hlght_off[tb] - hl0 : 0;
  if (P == 0) return EPI_OK;                                  // no candidate row: every table of the group is empty
  const int64_t nbp = (int64_t)((P + 255) / 256);
  EPI_TRY(check_grid(nbp, 256, "epi_batch_extract_patterns_multi"));
  c.st->pairs += (int64_t)P;

  // pass 1: overlap flags and position counts, the flags scanned into pattern slots
  const size_t nbase = ((size_t)ng + 2) & ~(size_t)1;         // base[ng + 1] (padded to an even count), then the counts
  EPI_TRY(w.meta.ensure(meta.size() * 8));
  EPI_TRY(w.flag.ensure((size_t)P * 4));
  EPI_TRY(w.cidx.ensure((size_t)P * 4));
  EPI_TRY(w.cb.ensure((nbase + (size_t)W) * 4));
  w.note();
  EPI_HIP(hipMemcpyAsync(w.meta.p, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, s));
  EPI_HIP(hipMemsetAsync(w.cb.p, 0, (nbase + (size_t)W) * 4, s));
  PatMulti m = c.m;
  m.pre = w.meta.as<uint64_t>();
  m.tg = reinterpret_cast<const PatTarget *>(w.meta.as<uint64_t>() + ng + 1);
  m.ng = ng;
  uint32_t *d_base = w.cb.as<uint32_t>(), *d_cnt = d_base + nbase;
  prof_begin("extract_patterns_multi", s);
  hipLaunchKernelGGL(k_patm_flag_count, dim3((unsigned)nbp), dim3(256), 0, s, m, P, w.flag.as<uint32_t>(), d_cnt);
  EPI_TRY(scan_exclusive_u32(w.flag.as<uint32_t>(), w.cidx.as<uint32_t>(), (int64_t)P, d_base + ng, b->scan_tmp, s));
  hipLaunchKernelGGL(k_patm_bases, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, s, m.pre, ng, P, w.cidx.as<uint32_t>(), d_base);
  EPI_HIP(hipGetLastError());
  prof_end("extract_patterns_multi", s);
  std::vector<uint32_t> h_cb(nbase + (size_t)W);
  EPI_HIP(hipMemcpyAsync(h_cb.data(), w.cb.p, h_cb.size() * 4, hipMemcpyDeviceToHost, s));
  EPI_HIP(hipStreamSynchronize(s));
  const uint32_t *h_base = h_cb.data(), *h_cnt = h_cb.data() + nbase;
  if (h_base[ng] == 0) return EPI_OK;                         // no row overlaps any target of the group

  // the host's decision for every target; cell batches of at most `cap` result bytes
  std::vector<std::vector<int32_t>> cols((size_t)ng);
  std::vector<int32_t> h_colmap((size_t)W, -1), h_hl((size_t)(2 * H + 2), 0);
  int32_t *h_hcol = h_hl.data() + H;
  if (H > 0) memcpy(h_hl.data(), c.hlght + hl0, (size_t)H * 4);
  std::vector<PatSlice> sl((size_t)ng);
  std::vector<PatSumSlice> ss(c.sum ? (size_t)ng : 0);
  std::vector<int32_t> cuts(1, 0);                            // batch i: targets [cuts[i], cuts[i + 1])
  int64_t bytes = 0, cell_off = 0, tab_off = 0;
  uint32_t rel = 0;
  for (int32_t k = 0; k < ng; k++) {
    const PatTarget &g = tg[k];
    const uint32_t npat0 = h_base[k + 1] - h_base[k];
    if (npat0) pat_choose_columns(h_cnt + g.win_off, g.nwin, g.pos_lo, npat0, c.min_ctx_freq, h_hl.data() + g.hl_off, g.nhl, cols[(size_t)k],
                                  h_colmap.data() + g.win_off, h_hcol + g.hl_off);
    const int64_t cells = (int64_t)cols[(size_t)k].size() * npat0;
    int64_t need = 32LL * npat0 + 4 * cells, tcap = 0;
    if (c.sum) {                                              // + its table slice, 20 B per slot and the unique rows at their most
      tcap = pat_table_capacity(npat0);
      need += 16 * tcap + 20LL * npat0 + 12LL * npat0 + 4 * cells;
    }
    if (bytes > 0 && bytes + need > c.cap) { cuts.push_back(k); bytes = 0; cell_off = 0; rel = 0; tab_off = 0; }
    sl[(size_t)k].cell_off = cell_off; sl[(size_t)k].base_abs = h_base[k]; sl[(size_t)k].base_rel = rel; sl[(size_t)k].npat0 = npat0; sl[(size_t)k].pad = 0;
    if (c.sum) { ss[(size_t)k].tab_off = tab_off; ss[(size_t)k].mask = tcap ? (uint32_t)(tcap - 1) : 0u; ss[(size_t)k].ncol = (uint32_t)cols[(size_t)k].size(); }
    bytes += need; cell_off += cells; rel += npat0; tab_off += tcap;
  }
  cuts.push_back(ng);
  EPI_TRY(w.colmap.ensure((size_t)W * 4));
  EPI_TRY(w.sl.ensure(sl.size() * sizeof(PatSlice)));
  EPI_TRY(w.hl.ensure(h_hl.size() * 4));
  if (c.sum) {
    EPI_TRY(w.ss.ensure(ss.size() * sizeof(PatSumSlice)));
    EPI_HIP(hipMemcpyAsync(w.ss.p, ss.data(), ss.size() * sizeof(PatSumSlice), hipMemcpyHostToDevice, s));
  }
  EPI_HIP(hipMemcpyAsync(w.colmap.p, h_colmap.data(), (size_t)W * 4, hipMemcpyHostToDevice, s));
  EPI_HIP(hipMemcpyAsync(w.sl.p, sl.data(), sl.size() * sizeof(PatSlice), hipMemcpyHostToDevice, s));
  EPI_HIP(hipMemcpyAsync(w.hl.p, h_hl.data(), h_hl.size() * 4, hipMemcpyHostToDevice, s));

  // pass 2, batch by batch: [fnv u64][nonempty, strand, start, end, nbase, meth i32] x slots, then the cells
  std::vector<uint64_t> h_res;
  for (size_t i = 0; i + 1 < cuts.size(); i++) {
    const int32_t sa = cuts[i], sb = cuts[i + 1];
    const size_t Ps = h_base[sb] - h_base[sa];
    if (Ps == 0) continue;
    size_t C = 0;
    for (int32_t k = sa; k < sb; k++) C += cols[(size_t)k].size() * sl[(size_t)k].npat0;
    const size_t rbytes = 32 * Ps + 4 * C;
    EPI_TRY(w.res.ensure(rbytes + 64));
    w.note();
    PatOut o;
    int32_t *ip = w.res.as<int32_t>();
    o.fnv = reinterpret_cast<unsigned long long *>(ip);
    int32_t *q = ip + 2 * Ps;
    o.nonempty = q; o.strand = q + Ps; o.start = q + 2 * Ps; o.end = q + 3 * Ps; o.nbase = q + 4 * Ps; o.meth = q + 5 * Ps;
    o.cells = q + 6 * Ps;
    if (C) EPI_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(o.cells), INT32_MIN, C, s));             // NA_INTEGER
    const uint64_t j0 = pre[sa], np = pre[sb] - pre[sa];
    prof_begin("extract_patterns_multi", s);
    hipLaunchKernelGGL(k_patm_extract, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, m, j0, np, w.flag.as<uint32_t>(),
                       w.cidx.as<uint32_t>(), w.sl.as<PatSlice>(), w.colmap.as<int32_t>(), w.hl.as<int32_t>(), w.hl.as<int32_t>() + H, o);
    EPI_HIP(hipGetLastError());
    prof_end("extract_patterns_multi", s);
    if (c.sum) {                                              // the slots stay on the device
      EPI_TRY(patm_summarise_batch(c, w, sl, ss, cols, ta, sa, sb, Ps, C, o));
      continue;
    }
    h_res.resize((rbytes + 7) / 8);
    EPI_HIP(hipMemcpyAsync(h_res.data(), w.res.p, rbytes, hipMemcpyDeviceToHost, s));
    EPI_HIP(hipStreamSynchronize(s));
    const unsigned long long *h_f = reinterpret_cast<const unsigned long long *>(h_res.data());
    const int32_t *r = reinterpret_cast<const int32_t *>(h_res.data()) + 2 * Ps, *h_cells = r + 6 * Ps;
    for (int32_t k = sa; k < sb; k++) {
      const PatSlice &q1 = sl[(size_t)k];
      if (!q1.npat0) continue;
      const int32_t *rk = r + q1.base_rel;
      EPI_TRY(pat_fill_table(c.out + ta + k, q1.npat0, (int32_t)cols[(size_t)k].size(), cols[(size_t)k].data(), rk, rk + Ps, rk + 2 * Ps,
                             rk + 3 * Ps, rk + 4 * Ps, rk + 5 * Ps, h_f + q1.base_rel, h_cells + q1.cell_off));
    }
  }
  return EPI_OK;
}

int patm_run(epi_batch *b, int32_t nt, const int32_t *t_rname, const int32_t *t_start, const int32_t *t_end, int32_t min_overlap,
             const char *ctx, double min_ctx_freq, int32_t clip, int32_t reverse_offset, const int32_t *hlght, const int64_t *hlght_off,
             void *stream, epi_pattern_table *out, epi_pattern_summary *sum, PatmStats &st) {
  EPI_HIP(hipSetDevice(b->eng->device));
  hipStream_t s = pick_stream(b, stream);
  EPI_TRY(fetch_row_stats(b, s));
  if (b->h_stats.bad_len) return fail(EPI_ERR_ARG, "offsets are not non-decreasing, or start+length exceeds int32");
  const int64_t lmax = b->h_stats.max_len;
  auto one_by_one = [&]() {                                   // rows in any order: every target scans the batch
    for (int32_t t = 0; t < nt; t++) {
      const int64_t h0 = hlght_off ? hlght_off[t] : 0, h1 = hlght_off ? hlght_off[t + 1] : 0;
      epi_pattern_table one;
      EPI_TRY(epi_batch_extract_patterns(b, t_rname[t], t_start[t], t_end[t], min_overlap, ctx, min_ctx_freq, clip, reverse_offset,
                                         h1 > h0 ? hlght + h0 : nullptr, (int32_t)(h1 - h0), stream, sum ? &one : out + t));
      if (!sum || !one.npat) continue;                        // the summary of a table: the host's grouping
      st.fallback++;
      const int rc = pat_summarise_host(sum + t, (size_t)one.npat, one.ncol, one.positions, nullptr, one.fnv, one.cells);
      epi_pattern_table_free(&one);
      EPI_TRY(rc);
    }
    return (int)EPI_OK;
  };
  bool ranges_ok = !b->h_stats.unsorted;
  std::vector<int64_t> pos_lo((size_t)nt), nwin((size_t)nt);
  for (int32_t t = 0; t < nt; t++) {
    if (t_start[t] < 0 || t_end[t] < 0) ranges_ok = false;    // (pat_span compares unsigned)
    pos_lo[(size_t)t] = (int64_t)t_start[t] - lmax - (int64_t)reverse_offset - 2;
    int64_t nw = ((int64_t)t_end[t] - (int64_t)t_start[t]) + 2 * lmax + (int64_t)reverse_offset + 8;
    if (nw < 1) nw = 1;
    if (nw > (1LL << 31)) return fail(EPI_ERR_ARG, "epi_batch_extract_patterns: target too wide");
    nwin[(size_t)t] = nw;
  }
  if (!ranges_ok) return one_by_one();

  // candidate rows of every target
  PatmScratch w;
  std::vector<int32_t> h_tgt((size_t)3 * nt);
  memcpy(h_tgt.data(), t_rname, (size_t)nt * 4);
  memcpy(h_tgt.data() + nt, t_start, (size_t)nt * 4);
  memcpy(h_tgt.data() + 2 * (size_t)nt, t_end, (size_t)nt * 4);
  std::vector<int64_t> h_rng((size_t)2 * nt + 1);
  EPI_TRY(w.tgt.ensure(h_tgt.size() * 4));
  EPI_TRY(w.rng.ensure(h_rng.size() * 8));
  w.note();
  EPI_HIP(hipMemcpyAsync(w.tgt.p, h_tgt.data(), h_tgt.size() * 4, hipMemcpyHostToDevice, s));
  EPI_HIP(hipMemsetAsync(w.rng.p, 0, h_rng.size() * 8, s));
  const int64_t reach = min_overlap >= 1 ? 0 : 1 - (int64_t)min_overlap;
  EPI_TRY(check_grid(((int64_t)nt + 255) / 256, 256, "epi_batch_extract_patterns_multi"));
  prof_begin("extract_patterns_multi", s);
  hipLaunchKernelGGL(k_patm_ranges, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, b->rname, b->start, b->n, w.tgt.as<int32_t>(), nt,
                     lmax, reach, w.rng.as<int64_t>());
  EPI_HIP(hipGetLastError());
  prof_end("extract_patterns_multi", s);
  EPI_HIP(hipMemcpyAsync(h_rng.data(), w.rng.p, h_rng.size() * 8, hipMemcpyDeviceToHost, s));
  EPI_HIP(hipStreamSynchronize(s));
  if (h_rng[(size_t)2 * nt]) return one_by_one();
  std::vector<int64_t> row_lo((size_t)nt), row_hi((size_t)nt);
  for (int32_t t = 0; t < nt; t++) { row_lo[(size_t)t] = h_rng[2 * (size_t)t]; row_hi[(size_t)t] = h_rng[2 * (size_t)t + 1]; }

  PatmCall c;
  c.b = b; c.s = s; c.t_rname = t_rname; c.t_start = t_start; c.t_end = t_end;
  c.row_lo = row_lo.data(); c.row_hi = row_hi.data(); c.pos_lo = pos_lo.data(); c.nwin = nwin.data();
  c.hlght = hlght; c.hlght_off = hlght_off; c.min_ctx_freq = min_ctx_freq; c.out = out; c.sum = sum; c.st = &st;
  const int hb = options().pat_hash_bits;
  c.key_mask = hb >= 1 && hb <= 63 ? (1ull << hb) - 1ull : ~0ull;
  c.cap = options().pat_group_bytes > 0 ? options().pat_group_bytes : kPatGroupBytes;
  c.m.xm = b->xm; c.m.off = b->off; c.m.len = b->len; c.m.rname = b->rname; c.m.strand = b->strand; c.m.start = b->start;
  c.m.reverse_offset = (uint32_t)reverse_offset; c.m.min_overlap = min_overlap; c.m.clip = clip ? 1 : 0;
  c.m.ctx_mask = 0;
  for (const unsigned char *p = reinterpret_cast<const unsigned char *>(ctx); *p; p++) c.m.ctx_mask |= 1u << ctx_to_idx(*p);
  c.m.tg = nullptr; c.m.pre = nullptr; c.m.ng = 0;

  // groups of consecutive targets whose pass-1 scratch (40 B per pair, 8 B per window position) fits the cap
  int rc = EPI_OK;
  for (int32_t ta = 0; ta < nt && rc == EPI_OK;) {
    int64_t bytes = 0;
    int32_t tb = ta;
    while (tb < nt) {
      const int64_t need = 40 * (row_hi[(size_t)tb] - row_lo[(size_t)tb]) + 8 * nwin[(size_t)tb] + 128;
      if (tb > ta && bytes + need > c.cap) break;
      bytes += need;
      tb++;
    }
    rc = patm_group(c, w, ta, tb);
    st.groups++;
    ta = tb;
  }
  if (w.peak > (size_t)st.scratch) st.scratch = (int64_t)w.peak;
  return rc;
}

// the arguments both multi-target entry points take
int patm_check_args(const char *what, const epi_batch *b, int32_t ntargets, const int32_t *target_rname, const int32_t *target_start,
                    const int32_t *target_end, const char *ctx, const int32_t *hlght, const int64_t *hlght_off, const void *out) {
  if (!b || !ctx || ntargets < 0 || (ntargets > 0 && (!target_rname || !target_start || !target_end || !out)))
    return fail(EPI_ERR_ARG, "%s: bad arguments", what);
  if (hlght_off) {
    for (int32_t t = 0; t < ntargets; t++)
      if (hlght_off[t] < 0 || hlght_off[t + 1] < hlght_off[t] || hlght_off[t + 1] - hlght_off[t] > 0x7FFFFFFF)
        return fail(EPI_ERR_ARG, "%s: hlght_off is not a CSR offset array", what);
    if (ntargets > 0 && hlght_off[ntargets] > hlght_off[0] && !hlght) return fail(EPI_ERR_ARG, "%s: hlght is NULL", what);
  }
  return EPI_OK;
}

}  // namespace

extern "C" {

int epi_batch_extract_patterns_multi(epi_batch *b, int32_t ntargets, const int32_t *target_rname, const int32_t *target_start,
                                     const int32_t *target_end, int32_t min_overlap, const char *ctx, double min_ctx_freq, int32_t clip,
                                     int32_t reverse_offset, const int32_t *hlght, const int64_t *hlght_off, void *stream,
                                     epi_pattern_table *out) {
  if (ntargets > 0 && out) memset(out, 0, (size_t)ntargets * sizeof(*out));
  EPI_TRY(patm_check_args("epi_batch_extract_patterns_multi", b, ntargets, target_rname, target_start, target_end, ctx, hlght, hlght_off, out));
  b->patm_groups = 0; b->patm_pairs = 0; b->patm_scratch = 0;
  if (ntargets == 0 || b->n == 0) return EPI_OK;
  PatmStats st;
  const int rc = patm_run(b, ntargets, target_rname, target_start, target_end, min_overlap, ctx, min_ctx_freq, clip, reverse_offset,
                          hlght, hlght_off, stream, out, nullptr, st);
  b->patm_groups = st.groups; b->patm_pairs = st.pairs; b->patm_scratch = st.scratch;
  if (rc != EPI_OK)
    for (int32_t t = 0; t < ntargets; t++) epi_pattern_table_free(out + t);
  return rc;
}

void epi_pattern_summary_free(epi_pattern_summary *t) {
  if (!t) return;
  free(t->positions); free(t->fnv); free(t->count); free(t->cells);
  memset(t, 0, sizeof(*t));
}

int epi_batch_summarise_patterns_multi(epi_batch *b, int32_t ntargets, const int32_t *target_rname, const int32_t *target_start,
                                       const int32_t *target_end, int32_t min_overlap, const char *ctx, double min_ctx_freq,
                                       int32_t clip, int32_t reverse_offset, const int32_t *hlght, const int64_t *hlght_off,
                                       void *stream, epi_pattern_summary *out) {
  if (ntargets > 0 && out) memset(out, 0, (size_t)ntargets * sizeof(*out));
  EPI_TRY(patm_check_args("epi_batch_summarise_patterns_multi", b, ntargets, target_rname, target_start, target_end, ctx, hlght, hlght_off, out));
  b->pats_groups = 0; b->pats_pairs = 0; b->pats_fallback = 0;
  if (ntargets == 0 || b->n == 0) return EPI_OK;
  PatmStats st;
  const int rc = patm_run(b, ntargets, target_rname, target_start, target_end, min_overlap, ctx, min_ctx_freq, clip, reverse_offset,
                          hlght, hlght_off, stream, nullptr, out, st);
  b->pats_groups = st.groups; b->pats_pairs = st.pairs; b->pats_fallback = st.fallback;
  if (rc != EPI_OK)
    for (int32_t t = 0; t < ntargets; t++) epi_pattern_summary_free(out + t);
  return rc;
}

int epi_batch_summarise_patterns_stats(epi_batch *b, int64_t *groups, int64_t *pairs, int64_t *fallback_targets) {
  if (!b) return fail(EPI_ERR_ARG, "epi_batch_summarise_patterns_stats: batch is NULL");
  if (groups) *groups = b->pats_groups;
  if (pairs) *pairs = b->pats_pairs;
  if (fallback_targets) *fallback_targets = b->pats_fallback;
  return EPI_OK;
}

int epi_batch_extract_patterns_multi_stats(epi_batch *b, int64_t *groups, int64_t *pairs, int64_t *scratch_bytes) {
  if (!b) return fail(EPI_ERR_ARG, "epi_batch_extract_patterns_multi_stats: batch is NULL");
  if (groups) *groups = b->patm_groups;
  if (pairs) *pairs = b->patm_pairs;
  if (scratch_bytes) *scratch_bytes = b->patm_scratch;
  return EPI_OK;
}

}  // extern "C"
