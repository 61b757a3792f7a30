// rcpp_extract_patterns (src/rcpp_extract_patterns.cpp:26-211): methylation patterns of the reads that overlap a target
// region, for one target (epi_batch_extract_patterns) or every target of a list (epi_batch_extract_patterns_multi).  The
// work is confined to the targets (a few thousand reads each), so this is two small passes around one host decision,
// not a bandwidth problem.  One path serves both calls: a GROUP of targets, each with a range of candidate rows; the
// ranges laid end to end are one flat list of (target, candidate row) pairs.
//   k_patm_ranges      rows sorted by (rname, start): one lane per target finds its candidate rows by search
//   k_patm_flag_count  pass 1, one thread per pair: does the read overlap its target by min_overlap (:79-86)?  -> scan ->
//                      its slot; and how often is each in-context position seen (:87-96)
//   host               valid positions = seen in >= min_ctx_freq of the overlapping reads and not highlighted (:103-108),
//                      merged with the highlight positions, ordered (:185)
//   k_patm_extract     pass 2, one thread per overlapping pair: its cell per valid position, methylated / total counts and
//                      the FNV-1a hash of (position, base) pairs, highlighted bases appended (:133-166)
//   host               drops empty patterns (:152) and returns the tables.
// A list whose rows are sorted and whose coordinates are not negative runs as groups of ranged targets, in O(1) launches
// and host round trips per group.  The single call, and every target of any other list, is a group of ONE target whose
// candidate rows are all rows [0, n): pat_span rejects the rows of other rnames itself, so neither pass relies on the range
// being tight.  epi_batch_summarise_patterns_multi runs the same two passes and then groups every target's patterns on
// the device (k_pats_*): only the unique patterns and their counts come to the host.
// Quirks of the reference kept as they are: with clip=TRUE the byte loop ends at `overlap`,
// not at begin+overlap (:86,:132), and position bytes enter the hash sign-extended (char pointer, epialleleR.h:8-13).
#include "common.hpp"
#include "pat_search.hpp"
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <unordered_map>
#include <vector>

namespace epi {

// The ranges of a group of targets are laid end to end as one flat list of (target, candidate row) pairs; pre[] is the
// u64 exclusive scan of the range lengths, and thread j finds its target as the last t with pre[t] <= j.  flag / cidx
// are indexed by pair, cnt / colmap by the targets' windows laid end to end: every target owns a slice of each.
struct PatTarget {
  int64_t row_lo;                 // its candidate rows: row_lo + (j - pre[t])
  int64_t pos_lo, nwin;           // window of positions that can occur: [pos_lo, pos_lo + nwin)
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
  const int64_t *off;             // row x owns xm[off[x] .. off[x] + len[x])
  const int32_t *len, *rname, *strand, *start;
  uint32_t reverse_offset, ctx_mask;
  int32_t min_overlap, clip;
  const PatTarget *tg;
  const uint64_t *pre;            // [ng + 1]
  int32_t ng;
};

struct PatSpan { uint32_t start_x, begin_i, end_i, offset_x; bool ok; };

__device__ __forceinline__ PatSpan pat_span(const PatMulti &m, const PatTarget &g, int64_t x) {
  PatSpan s;
  s.ok = false; s.start_x = 0; s.begin_i = 0; s.end_i = 0; s.offset_x = 0;
  if (m.rname[x] != g.rname) return s;                                      // :78
  const uint32_t target_start = (uint32_t)g.start, target_end = (uint32_t)g.end;
  const uint32_t size_x = (uint32_t)m.len[x];
  const uint32_t start_x = (uint32_t)m.start[x];
  const uint32_t end_x = start_x + size_x - 1u;
  const uint32_t over_start = start_x > target_start ? start_x : target_start;
  const uint32_t over_end = end_x < target_end ? end_x : target_end;
  const int32_t overlap = (int32_t)(over_end - over_start + 1u);            // :84
  if (overlap < m.min_overlap) return s;
  s.ok = true;
  s.start_x = start_x;
  s.offset_x = m.strand[x] == 2 ? m.reverse_offset : 0u;
  s.begin_i = m.clip ? over_start - start_x : 0u;
  s.end_i = m.clip ? (uint32_t)overlap : size_x;
  if (s.end_i > size_x) s.end_i = size_x;                                   // (the reference would read past the string)
  return s;
}

// row x overlaps the target (s = pat_span(m, g, x), s.ok): one count per in-context position of its span
__device__ __forceinline__ void pat_count_row(const PatMulti &m, const PatTarget &g, int64_t x, const PatSpan &s, uint32_t *__restrict__ cnt) {
  const uint8_t *p = m.xm + m.off[x];
  for (uint32_t i = s.begin_i; i < s.end_i; i++) {
    if (!((m.ctx_mask >> (p[i] & 15u)) & 1u)) continue;
    const int64_t w = (int64_t)(int32_t)(s.start_x + i - s.offset_x) - g.pos_lo;
    if (w >= 0 && w < g.nwin) atomicAdd(cnt + w, 1u);
  }
}

struct PatOut {
  int32_t *nonempty, *strand, *start, *end, *nbase, *meth;
  unsigned long long *fnv;
  int32_t *cells;                 // [ncol][npat0]
  // a target's part of a batch of results: its slots begin at `rel`, its cells at `cell_off`
  __host__ __device__ PatOut of(uint32_t rel, int64_t cell_off) const {
    PatOut t;
    t.nonempty = nonempty + rel; t.strand = strand + rel; t.start = start + rel; t.end = end + rel;
    t.nbase = nbase + rel; t.meth = meth + rel; t.fnv = fnv + rel;
    t.cells = cells + cell_off;
    return t;
  }
};

__device__ __forceinline__ void fnv_char(unsigned long long &h, uint32_t v) {   // four bytes through a (signed) char pointer
#pragma unroll
  for (int k = 0; k < 4; k++) {
    h ^= (unsigned long long)(long long)(signed char)((v >> (8 * k)) & 0xFFu);
    h *= 1099511628211ull;
  }
}

// row x overlaps the target (s = pat_span(m, g, x), s.ok) and is its c-th overlapping row: cells, counts and hash
__device__ __forceinline__ void pat_extract_row(const PatMulti &m, const PatTarget &g, int64_t x, const PatSpan &s, uint32_t c,
                                                const int32_t *__restrict__ colmap, const int32_t *__restrict__ hlght,
                                                const int32_t *__restrict__ hcol, int64_t npat0, const PatOut &o) {
  const uint8_t *p = m.xm + m.off[x];
  uint32_t meth = 0, total = 0;
  unsigned long long fnv = 14695981039346656037ull;
  for (uint32_t i = s.begin_i; i < s.end_i; i++) {
    const uint32_t base = p[i] & 15u;
    if (!((m.ctx_mask >> base) & 1u)) continue;
    const uint32_t pos = s.start_x + i - s.offset_x;
    const int64_t w = (int64_t)(int32_t)pos - g.pos_lo;
    if (w < 0 || w >= g.nwin) continue;
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
    for (int32_t k = 0; k < g.nhl; k++) {                                    // :154-164
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
  o.strand[c] = m.strand[x];
  o.start[c] = (int32_t)(s.start_x + s.begin_i);
  o.end[c] = (int32_t)(s.start_x + s.end_i - 1u);
  o.nbase[c] = (int32_t)total;
  o.meth[c] = (int32_t)meth;
  o.fnv[c] = fnv;
}

// Rows sorted by (rname, start), one lane per target: rng[2t], rng[2t+1] = its candidate rows, those on its rname that
// start in [start - reach - lmax + 1, end + reach] (reach = 0 for min_overlap >= 1: pat_span accepts no other row).
// rng[2 * nt] != 0: some target's rname holds a row with a negative start (pat_span's unsigned arithmetic lets such a
// row overlap anything; the caller runs every target against all rows).
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
  const int64_t x = g.row_lo + (int64_t)(j - m.pre[t]);
  const PatSpan s = pat_span(m, g, x);
  flag[j] = s.ok ? 1u : 0u;
  if (s.ok) pat_count_row(m, g, x, s, cnt + g.win_off);
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
  const int64_t x = g.row_lo + (int64_t)(j - m.pre[t]);
  pat_extract_row(m, g, x, pat_span(m, g, x), cidx[j] - q.base_abs, colmap + g.win_off, hl + g.hl_off, hcol + g.hl_off, (int64_t)q.npat0,
                  o.of(q.base_rel, q.cell_off));
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
  return pat_last_le(sa, sb, i, [&](int32_t t) { return sl[t].base_rel; });
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

// ---- the host side -------------------------------------------------------------------------------------------------------
namespace {

constexpr int64_t kPatGroupBytes = 256LL << 20;   // scratch cap of a group of targets (include/epihip.h)

enum PatBuf {                     // the device scratch of a call
  kTgt, kRng, kMeta, kFlag, kCidx, kCb, kColmap, kSl, kHl, kRes,
  kSs, kTab, kSlot, kUb, kSout,   // the summary path: table slices, table, 5 x u32 per slot, bases and collide words, output
  kPatBufs
};
struct PatmScratch {
  DevBuf buf[kPatBufs];
  size_t peak = 0;
  DevBuf &operator[](PatBuf i) { return buf[i]; }
  void note() {
    size_t v = 0;
    for (const DevBuf &d : buf) v += d.cap;
    if (v > peak) peak = v;
  }
};

struct PatmStats { int64_t groups = 0, pairs = 0, scratch = 0, fallback = 0; };

struct PatmCall {                 // what every group of a call shares
  epi_batch *b;
  hipStream_t s;
  const char *entry, *label;      // whose errors and whose profiler label the launches go under
  const int32_t *t_rname, *t_start, *t_end;
  const int64_t *rng;             // [2 * ntargets] the candidate rows of target t: [rng[2t], rng[2t + 1])
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

struct PatGroup {                 // targets [ta, ta + ng) of a call, as the steps of patm_group hand them on
  int32_t ta = 0, ng = 0;
  std::vector<uint64_t> meta;     // as the device reads it: pre[ng + 1], then tg[ng]
  const uint64_t *pre = nullptr;
  const PatTarget *tg = nullptr;
  int64_t W = 0, H = 0, hl0 = 0;  // window and highlight positions of the group; its first highlight position in c.hlght
  PatMulti m;                     // the call's, with the group's pre / tg on the device
  size_t nbase = 0;               // base[ng + 1], padded to an even count
  std::vector<uint32_t> h_cb;     // pass 1, fetched: base[nbase], cnt[W]
  std::vector<std::vector<int32_t>> cols;   // the plan: per target its column positions,
  std::vector<int32_t> h_colmap, h_hl;      // colmap[W]; hl[H], hcol[H],
  std::vector<PatSlice> sl;
  std::vector<PatSumSlice> ss;    // (summaries only)
  std::vector<int32_t> cuts;      // and cell batch i: targets [cuts[i], cuts[i + 1])
  const uint32_t *h_base() const { return h_cb.data(); }
  const uint32_t *h_cnt() const { return h_cb.data() + nbase; }
};

struct PatBatch {                 // a cell batch: targets [sa, sb) of a group, their Ps slots and C cells, in `o` after pass 2
  int32_t sa, sb;
  size_t Ps, C;
  PatOut o;
};

// the per-slot arrays and the cells of ns slots in one buffer: [fnv u64][nonempty, strand, start, end, nbase, meth i32] x ns, cells
PatOut pat_out_at(void *base, size_t ns) {
  PatOut o;
  o.fnv = reinterpret_cast<unsigned long long *>(base);                // 8-byte aligned first
  int32_t *q = reinterpret_cast<int32_t *>(base) + 2 * ns;
  o.nonempty = q; o.strand = q + ns; o.start = q + 2 * ns; o.end = q + 3 * ns; o.nbase = q + 4 * ns; o.meth = q + 5 * ns;
  o.cells = q + 6 * ns;
  return o;
}

// the longest row (it bounds the window of positions); refuses a batch whose rows are not well-formed
int pat_longest_row(epi_batch *b, hipStream_t s, int64_t *lmax) {
  EPI_TRY(fetch_row_stats(b, s));
  if (b->h_stats.bad_len) return fail(EPI_ERR_ARG, "offsets are not non-decreasing, or start+length exceeds int32");
  *lmax = b->h_stats.max_len;
  return EPI_OK;
}

// the window of positions the rows that overlap a target can name: [pos_lo, pos_lo + nwin)
int pat_window(int32_t start, int32_t end, int64_t lmax, int32_t reverse_offset, int64_t *pos_lo, int64_t *nwin) {
  *pos_lo = (int64_t)start - lmax - (int64_t)reverse_offset - 2;
  *nwin = ((int64_t)end - (int64_t)start) + 2 * lmax + (int64_t)reverse_offset + 8;
  if (*nwin < 1) *nwin = 1;
  if (*nwin > (1LL << 31)) return fail(EPI_ERR_ARG, "epi_batch_extract_patterns: target too wide");
  return EPI_OK;
}

// what a call's groups share, but for its targets, results and statistics
PatmCall patm_call(epi_batch *b, hipStream_t s, int32_t min_overlap, const char *ctx, double min_ctx_freq, int32_t clip,
                   int32_t reverse_offset) {
  PatmCall c = {};
  c.b = b; c.s = s; c.min_ctx_freq = min_ctx_freq;
  c.entry = "epi_batch_extract_patterns_multi"; c.label = "extract_patterns_multi";
  const int hb = options().pat_hash_bits;
  c.key_mask = hb >= 1 && hb <= 63 ? (1ull << hb) - 1ull : ~0ull;
  c.cap = options().pat_group_bytes > 0 ? options().pat_group_bytes : kPatGroupBytes;
  c.m.xm = b->xm; c.m.off = b->off; c.m.len = b->len; c.m.rname = b->rname; c.m.strand = b->strand; c.m.start = b->start;
  c.m.reverse_offset = (uint32_t)reverse_offset; c.m.min_overlap = min_overlap; c.m.clip = clip ? 1 : 0;
  c.m.ctx_mask = ctx_mask_of(ctx);
  return c;
}

// The host's decision between the two passes: valid positions = seen in >= min_ctx_freq of the npat0 overlapping reads
// and not highlighted (:103-108), the highlight positions (:110-112), merged in position order (:185).  cnt / colmap:
// the nwin positions from pos_lo on (colmap: column of a valid position, else -1); hcol[k]: column of hlght[k].
void pat_choose_columns(const uint32_t *cnt, int64_t nwin, int64_t pos_lo, uint32_t npat0, double min_ctx_freq,
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

// The table of one target from the P0 slots its overlapping rows filled (o: on the host, cells [ncol][P0]): keeps the
// non-empty patterns, in row order (:152, :166-176).
int pat_fill_table(epi_pattern_table *out, size_t P0, int32_t ncol, const int32_t *cols, const PatOut &o) {
  size_t np = 0;
  for (size_t c = 0; c < P0; c++) np += o.nonempty[c] != 0;
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
    if (!o.nonempty[c]) continue;
    out->strand[w] = o.strand[c]; out->start[w] = o.start[c]; out->end[w] = o.end[c];
    out->nbase[w] = o.nbase[c];
    out->beta[w] = (double)(uint32_t)o.meth[c] / (uint32_t)o.nbase[c];                            // :173
    out->fnv[w] = o.fnv[c];
    for (int32_t k = 0; k < ncol; k++) out->cells[(size_t)k * np + w] = o.cells[(size_t)k * P0 + c];
    w++;
  }
  return EPI_OK;
}

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

// ---- the summaries of a cell batch ---------------------------------------------------------------------------------------
// Groups the batch's slots on the device: table, verify, scans and emit.  Fetches ubase[nb + 1], wbase[nb + 1] and the
// collide words [nb] into h_ub.
int pats_group_fetch_counts(PatmCall &c, PatmScratch &w, const PatBatch &bt, int64_t TE, std::vector<uint32_t> &h_ub) {
  hipStream_t s = c.s;
  const int32_t nb = bt.sb - bt.sa;
  const size_t Ps = bt.Ps;
  const int64_t nbs = (int64_t)((Ps + 255) / 256), nbt = (TE + 255) / 256;
  EPI_TRY(check_grid(nbs, 256, "epi_batch_summarise_patterns_multi"));
  EPI_TRY(check_grid(nbt, 256, "epi_batch_summarise_patterns_multi"));
  EPI_TRY(w[kTab].ensure((size_t)TE * sizeof(PatEntry)));
  EPI_TRY(w[kSlot].ensure(5 * Ps * 4));
  EPI_TRY(w[kUb].ensure(h_ub.size() * 4));
  EPI_TRY(w[kSout].ensure(12 * Ps + 4 * bt.C + 16));
  w.note();
  uint32_t *ent = w[kSlot].as<uint32_t>(), *first = ent + Ps, *wfirst = ent + 2 * Ps, *uidx = ent + 3 * Ps, *widx = ent + 4 * Ps;
  uint32_t *ubase = w[kUb].as<uint32_t>(), *wbase = ubase + nb + 1, *collide = wbase + nb + 1;
  PatSum q;
  q.sl = w[kSl].as<PatSlice>(); q.ss = w[kSs].as<PatSumSlice>(); q.sa = bt.sa; q.sb = bt.sb; q.nslot = (uint32_t)Ps;
  q.fnv = bt.o.fnv; q.nonempty = bt.o.nonempty; q.cells = bt.o.cells;
  q.tab = w[kTab].as<PatEntry>(); q.ent = ent; q.collide = collide; q.key_mask = c.key_mask;
  EPI_HIP(hipMemsetAsync(w[kUb].p, 0, h_ub.size() * 4, s));
  prof_begin("summarise_patterns", s);
  hipLaunchKernelGGL(k_pats_init, dim3((unsigned)nbt), dim3(256), 0, s, q.tab, TE);
  prof_begin("summarise_patterns_insert", s);
  hipLaunchKernelGGL(k_pats_insert, dim3((unsigned)nbs), dim3(256), 0, s, q);
  prof_end("summarise_patterns_insert", s);
  hipLaunchKernelGGL(k_pats_verify, dim3((unsigned)nbs), dim3(256), 0, s, q, first, wfirst);
  EPI_TRY(scan_exclusive_u32(first, uidx, (int64_t)Ps, ubase + nb, c.b->scan_tmp, s));
  EPI_TRY(scan_exclusive_u32(wfirst, widx, (int64_t)Ps, wbase + nb, c.b->scan_tmp, s));
  hipLaunchKernelGGL(k_pats_bases, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, q.sl, bt.sa, nb, q.nslot, uidx, widx, ubase, wbase);
  hipLaunchKernelGGL(k_pats_emit, dim3((unsigned)nbs), dim3(256), 0, s, q, first, uidx, ubase, wbase, w[kSout].as<unsigned long long>());
  EPI_HIP(hipGetLastError());
  prof_end("summarise_patterns", s);
  EPI_HIP(hipMemcpyAsync(h_ub.data(), w[kUb].p, h_ub.size() * 4, hipMemcpyDeviceToHost, s));
  EPI_HIP(hipStreamSynchronize(s));
  return EPI_OK;
}

// Fetches the U unique rows the device emitted: [fnv u64 x U][count u32 x U][cells i32, per target [ncol][nuniq]]
int pats_fetch_unique_rows(PatmCall &c, PatmScratch &w, const PatBatch &bt, const std::vector<uint32_t> &h_ub, std::vector<uint64_t> &h_out) {
  const size_t nb = (size_t)(bt.sb - bt.sa), U = h_ub[nb], WC = h_ub[2 * nb + 1];
  if (U > bt.Ps || WC > bt.C) return fail(EPI_ERR_STATE, "epi_batch_summarise_patterns_multi: more unique rows than slots");
  h_out.resize((12 * U + 4 * WC + 7) / 8 + 1);
  if (!U) return EPI_OK;
  EPI_HIP(hipMemcpyAsync(h_out.data(), w[kSout].p, 12 * U + 4 * WC, hipMemcpyDeviceToHost, c.s));
  EPI_HIP(hipStreamSynchronize(c.s));
  return EPI_OK;
}

// The summaries of the batch's targets from the device's unique rows.  -> regroup: the targets in which two patterns share
// a key, or all of them when the batch was too large for the device's indices; counted as grouped on the host.
int pats_fill_from_device(PatmCall &c, const PatGroup &g, const PatBatch &bt, bool on_device, const std::vector<uint32_t> &h_ub,
                          const std::vector<uint64_t> &h_out, std::vector<int32_t> &regroup) {
  const int32_t nb = bt.sb - bt.sa;
  const uint32_t *ubase = h_ub.data(), *wbase = ubase + nb + 1, *collide = wbase + nb + 1;
  const size_t U = ubase[nb];
  const uint64_t *u_fnv = h_out.data();
  const int32_t *u_count = reinterpret_cast<const int32_t *>(h_out.data() + U), *u_cells = u_count + U;
  for (int32_t k = bt.sa; k < bt.sb; k++) {
    if (!g.sl[(size_t)k].npat0) continue;
    if (!on_device || collide[k - bt.sa]) {
      c.st->fallback++;
      regroup.push_back(k);
      continue;
    }
    const std::vector<int32_t> &ck = g.cols[(size_t)k];
    const uint32_t u0 = ubase[k - bt.sa];
    EPI_TRY(pat_fill_summary(c.sum + g.ta + k, ubase[k - bt.sa + 1] - u0, (int32_t)ck.size(), ck.data(), u_fnv + u0, u_count + u0,
                             u_cells + wbase[k - bt.sa]));
  }
  return EPI_OK;
}

// The summaries of the targets of `regroup` by the host's grouping: fetches the slots pass 2 left for them
int pats_regroup_on_host(PatmCall &c, const PatGroup &g, const PatBatch &bt, const std::vector<int32_t> &regroup) {
  struct Slots { std::vector<uint64_t> fnv; std::vector<int32_t> nonempty, cells; };
  std::vector<Slots> back(regroup.size());
  for (size_t i = 0; i < regroup.size(); i++) {
    const PatSlice &q = g.sl[(size_t)regroup[i]];
    const size_t n0 = q.npat0, ncol = g.cols[(size_t)regroup[i]].size();
    Slots &f = back[i];
    f.fnv.resize(n0); f.nonempty.resize(n0); f.cells.resize(ncol * n0 + 1);
    EPI_HIP(hipMemcpyAsync(f.fnv.data(), bt.o.fnv + q.base_rel, n0 * 8, hipMemcpyDeviceToHost, c.s));
    EPI_HIP(hipMemcpyAsync(f.nonempty.data(), bt.o.nonempty + q.base_rel, n0 * 4, hipMemcpyDeviceToHost, c.s));
    if (ncol) EPI_HIP(hipMemcpyAsync(f.cells.data(), bt.o.cells + q.cell_off, ncol * n0 * 4, hipMemcpyDeviceToHost, c.s));
  }
  EPI_HIP(hipStreamSynchronize(c.s));
  for (size_t i = 0; i < regroup.size(); i++) {
    const std::vector<int32_t> &ck = g.cols[(size_t)regroup[i]];
    EPI_TRY(pat_summarise_host(c.sum + g.ta + regroup[i], g.sl[(size_t)regroup[i]].npat0, (int32_t)ck.size(), ck.data(), back[i].nonempty.data(),
                               back[i].fnv.data(), back[i].cells.data()));
  }
  return EPI_OK;
}

// The summaries of a batch whose slots pass 2 has just left on the device: two host synchronisations (the counts, the
// unique rows) and a third when targets are regrouped on the host (their slots).
int patm_summarise_batch(PatmCall &c, PatmScratch &w, const PatGroup &g, const PatBatch &bt) {
  const int32_t nb = bt.sb - bt.sa;
  int64_t TE = 0;
  for (int32_t k = bt.sa; k < bt.sb; k++) TE += pat_table_capacity(g.sl[(size_t)k].npat0);
  const bool on_device = bt.Ps < (1u << 30) && bt.C < (1u << 31) && TE < (1LL << 32);    // u32 slot and cell indices
  std::vector<uint32_t> h_ub(3 * (size_t)nb + 2, 0);          // ubase[nb + 1], wbase[nb + 1], collide[nb]
  std::vector<uint64_t> h_out;
  if (on_device) {
    EPI_TRY(pats_group_fetch_counts(c, w, bt, TE, h_ub));
    EPI_TRY(pats_fetch_unique_rows(c, w, bt, h_ub, h_out));
  } else {
    EPI_HIP(hipStreamSynchronize(c.s));
  }
  std::vector<int32_t> regroup;
  EPI_TRY(pats_fill_from_device(c, g, bt, on_device, h_ub, h_out, regroup));
  return regroup.empty() ? EPI_OK : pats_regroup_on_host(c, g, bt, regroup);
}

// ---- a group of targets ----------------------------------------------------------------------------------------------------
// what the device reads of targets [ta, tb): every target's rows, window and highlight positions, the pairs before it
void patm_layout(const PatmCall &c, int32_t ta, int32_t tb, PatGroup &g) {
  const int32_t ng = tb - ta;
  g.ta = ta; g.ng = ng;
  g.meta.assign((size_t)(ng + 1) + ((size_t)ng * sizeof(PatTarget) + 7) / 8, 0);
  uint64_t *pre = g.meta.data();
  PatTarget *tg = reinterpret_cast<PatTarget *>(g.meta.data() + ng + 1);
  g.hl0 = c.hlght_off ? c.hlght_off[ta] : 0;
  g.H = c.hlght_off ? c.hlght_off[tb] - g.hl0 : 0;
  g.W = 0;
  pre[0] = 0;
  for (int32_t k = 0; k < ng; k++) {
    const int32_t t = ta + k;
    PatTarget &q = tg[k];
    q.row_lo = c.rng[2 * (size_t)t]; q.pos_lo = c.pos_lo[t]; q.nwin = c.nwin[t]; q.win_off = g.W;
    q.hl_off = c.hlght_off ? c.hlght_off[t] - g.hl0 : 0;
    q.nhl = c.hlght_off ? (int32_t)(c.hlght_off[t + 1] - c.hlght_off[t]) : 0;
    q.rname = c.t_rname[t]; q.start = c.t_start[t]; q.end = c.t_end[t];
    g.W += q.nwin;
    pre[k + 1] = pre[k] + (uint64_t)(c.rng[2 * (size_t)t + 1] - c.rng[2 * (size_t)t]);
  }
  g.pre = pre; g.tg = tg;
}

// Pass 1: overlap flags and position counts, the flags scanned into pattern slots.  Fetches every target's first slot and
// the counts of its window into g.h_cb.
int patm_pass1_fetch_counts(PatmCall &c, PatmScratch &w, PatGroup &g) {
  hipStream_t s = c.s;
  const int32_t ng = g.ng;
  const uint64_t P = g.pre[ng];
  const int64_t nbp = (int64_t)((P + 255) / 256);
  EPI_TRY(check_grid(nbp, 256, c.entry));
  c.st->pairs += (int64_t)P;
  g.nbase = ((size_t)ng + 2) & ~(size_t)1;                    // (the counts follow base[] in one buffer)
  g.h_cb.resize(g.nbase + (size_t)g.W);
  EPI_TRY(w[kMeta].ensure(g.meta.size() * 8));
  EPI_TRY(w[kFlag].ensure((size_t)P * 4));
  EPI_TRY(w[kCidx].ensure((size_t)P * 4));
  EPI_TRY(w[kCb].ensure(g.h_cb.size() * 4));
  w.note();
  EPI_HIP(hipMemcpyAsync(w[kMeta].p, g.meta.data(), g.meta.size() * 8, hipMemcpyHostToDevice, s));
  EPI_HIP(hipMemsetAsync(w[kCb].p, 0, g.h_cb.size() * 4, s));
  g.m = c.m;
  g.m.pre = w[kMeta].as<uint64_t>();
  g.m.tg = reinterpret_cast<const PatTarget *>(w[kMeta].as<uint64_t>() + ng + 1);
  g.m.ng = ng;
  uint32_t *d_base = w[kCb].as<uint32_t>(), *d_cnt = d_base + g.nbase;
  prof_begin(c.label, s);
  hipLaunchKernelGGL(k_patm_flag_count, dim3((unsigned)nbp), dim3(256), 0, s, g.m, P, w[kFlag].as<uint32_t>(), d_cnt);
  EPI_TRY(scan_exclusive_u32(w[kFlag].as<uint32_t>(), w[kCidx].as<uint32_t>(), (int64_t)P, d_base + ng, c.b->scan_tmp, s));
  hipLaunchKernelGGL(k_patm_bases, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, s, g.m.pre, ng, P, w[kCidx].as<uint32_t>(), d_base);
  EPI_HIP(hipGetLastError());
  prof_end(c.label, s);
  EPI_HIP(hipMemcpyAsync(g.h_cb.data(), w[kCb].p, g.h_cb.size() * 4, hipMemcpyDeviceToHost, s));
  EPI_HIP(hipStreamSynchronize(s));
  return EPI_OK;
}

// The host's decision for every target and the cell batches, consecutive targets whose results stay under the cap; queues
// the upload of what pass 2 reads of them
int patm_plan_upload(PatmCall &c, PatmScratch &w, PatGroup &g) {
  const size_t ng = (size_t)g.ng;
  g.cols.assign(ng, std::vector<int32_t>());
  g.h_colmap.assign((size_t)g.W, -1);
  g.h_hl.assign((size_t)(2 * g.H + 2), 0);
  int32_t *h_hcol = g.h_hl.data() + g.H;
  if (g.H > 0) memcpy(g.h_hl.data(), c.hlght + g.hl0, (size_t)g.H * 4);
  g.sl.assign(ng, PatSlice());
  g.ss.assign(c.sum ? ng : 0, PatSumSlice());
  g.cuts.assign(1, 0);
  const uint32_t *h_base = g.h_base();
  int64_t bytes = 0, cell_off = 0, tab_off = 0;
  uint32_t rel = 0;
  for (size_t k = 0; k < ng; k++) {
    const PatTarget &q = g.tg[k];
    const uint32_t npat0 = h_base[k + 1] - h_base[k];
    if (npat0) pat_choose_columns(g.h_cnt() + q.win_off, q.nwin, q.pos_lo, npat0, c.min_ctx_freq, g.h_hl.data() + q.hl_off, q.nhl, g.cols[k],
                                  g.h_colmap.data() + q.win_off, h_hcol + q.hl_off);
    const int64_t cells = (int64_t)g.cols[k].size() * npat0;
    int64_t need = 32LL * npat0 + 4 * cells, tcap = 0;
    if (c.sum) {                                              // + its table slice, 20 B per slot and the unique rows at their most
      tcap = pat_table_capacity(npat0);
      need += 16 * tcap + 20LL * npat0 + 12LL * npat0 + 4 * cells;
    }
    if (bytes > 0 && bytes + need > c.cap) { g.cuts.push_back((int32_t)k); bytes = 0; cell_off = 0; rel = 0; tab_off = 0; }
    PatSlice &sl = g.sl[k];
    sl.cell_off = cell_off; sl.base_abs = h_base[k]; sl.base_rel = rel; sl.npat0 = npat0; sl.pad = 0;
    if (c.sum) { g.ss[k].tab_off = tab_off; g.ss[k].mask = tcap ? (uint32_t)(tcap - 1) : 0u; g.ss[k].ncol = (uint32_t)g.cols[k].size(); }
    bytes += need; cell_off += cells; rel += npat0; tab_off += tcap;
  }
  g.cuts.push_back(g.ng);
  hipStream_t s = c.s;
  EPI_TRY(w[kColmap].ensure((size_t)g.W * 4));
  EPI_TRY(w[kSl].ensure(g.sl.size() * sizeof(PatSlice)));
  EPI_TRY(w[kHl].ensure(g.h_hl.size() * 4));
  if (c.sum) {
    EPI_TRY(w[kSs].ensure(g.ss.size() * sizeof(PatSumSlice)));
    EPI_HIP(hipMemcpyAsync(w[kSs].p, g.ss.data(), g.ss.size() * sizeof(PatSumSlice), hipMemcpyHostToDevice, s));
  }
  EPI_HIP(hipMemcpyAsync(w[kColmap].p, g.h_colmap.data(), (size_t)g.W * 4, hipMemcpyHostToDevice, s));
  EPI_HIP(hipMemcpyAsync(w[kSl].p, g.sl.data(), g.sl.size() * sizeof(PatSlice), hipMemcpyHostToDevice, s));
  EPI_HIP(hipMemcpyAsync(w[kHl].p, g.h_hl.data(), g.h_hl.size() * 4, hipMemcpyHostToDevice, s));
  return EPI_OK;
}

// Pass 2 of one cell batch: the slots and cells of its targets into bt.o (the result buffer, cells NA_INTEGER first)
int patm_pass2(PatmCall &c, PatmScratch &w, const PatGroup &g, PatBatch &bt) {
  hipStream_t s = c.s;
  EPI_TRY(w[kRes].ensure(32 * bt.Ps + 4 * bt.C + 64));
  w.note();
  bt.o = pat_out_at(w[kRes].p, bt.Ps);
  if (bt.C) EPI_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(bt.o.cells), INT32_MIN, bt.C, s));
  const uint64_t j0 = g.pre[bt.sa], np = g.pre[bt.sb] - g.pre[bt.sa];
  prof_begin(c.label, s);
  hipLaunchKernelGGL(k_patm_extract, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, g.m, j0, np, w[kFlag].as<uint32_t>(),
                     w[kCidx].as<uint32_t>(), w[kSl].as<PatSlice>(), w[kColmap].as<int32_t>(), w[kHl].as<int32_t>(), w[kHl].as<int32_t>() + g.H,
                     bt.o);
  EPI_HIP(hipGetLastError());
  prof_end(c.label, s);
  return EPI_OK;
}

// Fetches a batch's slots and cells (h_res: the call's staging buffer) and makes the tables of its targets
int patm_fetch_tables(PatmCall &c, PatmScratch &w, const PatGroup &g, const PatBatch &bt, std::vector<uint64_t> &h_res) {
  const size_t rbytes = 32 * bt.Ps + 4 * bt.C;
  h_res.resize((rbytes + 7) / 8);
  EPI_HIP(hipMemcpyAsync(h_res.data(), w[kRes].p, rbytes, hipMemcpyDeviceToHost, c.s));
  EPI_HIP(hipStreamSynchronize(c.s));
  const PatOut h = pat_out_at(h_res.data(), bt.Ps);
  for (int32_t k = bt.sa; k < bt.sb; k++) {
    const PatSlice &q = g.sl[(size_t)k];
    if (!q.npat0) continue;
    const std::vector<int32_t> &ck = g.cols[(size_t)k];
    EPI_TRY(pat_fill_table(c.out + g.ta + k, q.npat0, (int32_t)ck.size(), ck.data(), h.of(q.base_rel, q.cell_off)));
  }
  return EPI_OK;
}

// targets [ta, tb): two passes, two host synchronisations and one more per cell batch (the summaries: two or three per batch)
int patm_group(PatmCall &c, PatmScratch &w, int32_t ta, int32_t tb) {
  PatGroup g;
  patm_layout(c, ta, tb, g);
  if (g.pre[g.ng] == 0) return EPI_OK;                        // no candidate row: every table of the group is empty
  EPI_TRY(patm_pass1_fetch_counts(c, w, g));
  if (g.h_base()[g.ng] == 0) return EPI_OK;                   // no row overlaps any target of the group
  EPI_TRY(patm_plan_upload(c, w, g));
  std::vector<uint64_t> h_res;
  for (size_t i = 0; i + 1 < g.cuts.size(); i++) {
    PatBatch bt;
    bt.sa = g.cuts[i]; bt.sb = g.cuts[i + 1];
    bt.Ps = g.h_base()[bt.sb] - g.h_base()[bt.sa];
    if (bt.Ps == 0) continue;
    bt.C = 0;
    for (int32_t k = bt.sa; k < bt.sb; k++) bt.C += g.cols[(size_t)k].size() * g.sl[(size_t)k].npat0;
    EPI_TRY(patm_pass2(c, w, g, bt));
    EPI_TRY(c.sum ? patm_summarise_batch(c, w, g, bt) : patm_fetch_tables(c, w, g, bt, h_res));   // (a summary's slots stay on the device)
  }
  return EPI_OK;
}

// ---- a call ----------------------------------------------------------------------------------------------------------------
// Target t of the call alone against all rows [0, n), its table into `out`: what epi_batch_extract_patterns is.  Leaves the
// call's statistics alone; its launches go under the single call's label.
int patm_all_rows(const PatmCall &c, PatmScratch &w, int32_t t, epi_pattern_table *out) {
  const int64_t rows[2] = {0, c.b->n};
  PatmStats unused;
  PatmCall one = c;
  one.t_rname += t; one.t_start += t; one.t_end += t; one.pos_lo += t; one.nwin += t;
  if (one.hlght_off) one.hlght_off += t;
  one.rng = rows;
  one.out = out; one.sum = nullptr; one.st = &unused;
  one.entry = "epi_batch_extract_patterns"; one.label = "extract_patterns";
  return patm_group(one, w, 0, 1);
}

// Rows in any order, or coordinates below 0: every target scans the batch, cost O(rows x targets), one scratch for all.
// The summary of such a target is the host's grouping of its table.
int patm_target_by_target(const PatmCall &c, PatmScratch &w, int32_t nt) {
  for (int32_t t = 0; t < nt; t++) {
    epi_pattern_table one;
    memset(&one, 0, sizeof(one));
    EPI_TRY(patm_all_rows(c, w, t, c.sum ? &one : c.out + t));
    if (!c.sum || !one.npat) continue;
    c.st->fallback++;
    const int rc = pat_summarise_host(c.sum + t, (size_t)one.npat, one.ncol, one.positions, nullptr, one.fnv, one.cells);
    epi_pattern_table_free(&one);
    EPI_TRY(rc);
  }
  return EPI_OK;
}

// Rows sorted by (rname, start): fetches the candidate rows of every target, rng[2t], rng[2t + 1], and rng[2 * nt] != 0 when
// a target's rname holds a row with a negative start
int patm_fetch_candidate_rows(PatmCall &c, PatmScratch &w, int32_t nt, int64_t lmax, int32_t min_overlap, std::vector<int64_t> &h_rng) {
  hipStream_t s = c.s;
  std::vector<int32_t> h_tgt((size_t)3 * nt);
  memcpy(h_tgt.data(), c.t_rname, (size_t)nt * 4);
  memcpy(h_tgt.data() + nt, c.t_start, (size_t)nt * 4);
  memcpy(h_tgt.data() + 2 * (size_t)nt, c.t_end, (size_t)nt * 4);
  h_rng.resize((size_t)2 * nt + 1);
  EPI_TRY(w[kTgt].ensure(h_tgt.size() * 4));
  EPI_TRY(w[kRng].ensure(h_rng.size() * 8));
  w.note();
  EPI_HIP(hipMemcpyAsync(w[kTgt].p, h_tgt.data(), h_tgt.size() * 4, hipMemcpyHostToDevice, s));
  EPI_HIP(hipMemsetAsync(w[kRng].p, 0, h_rng.size() * 8, s));
  const int64_t reach = min_overlap >= 1 ? 0 : 1 - (int64_t)min_overlap;
  EPI_TRY(check_grid(((int64_t)nt + 255) / 256, 256, c.entry));
  prof_begin(c.label, s);
  hipLaunchKernelGGL(k_patm_ranges, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, c.b->rname, c.b->start, c.b->n, w[kTgt].as<int32_t>(), nt,
                     lmax, reach, w[kRng].as<int64_t>());
  EPI_HIP(hipGetLastError());
  prof_end(c.label, s);
  EPI_HIP(hipMemcpyAsync(h_rng.data(), w[kRng].p, h_rng.size() * 8, hipMemcpyDeviceToHost, s));
  EPI_HIP(hipStreamSynchronize(s));
  return EPI_OK;
}

int patm_run(epi_batch *b, int32_t nt, const int32_t *t_rname, const int32_t *t_start, const int32_t *t_end, int32_t min_overlap,
             const char *ctx, double min_ctx_freq, int32_t clip, int32_t reverse_offset, const int32_t *hlght, const int64_t *hlght_off,
             void *stream, epi_pattern_table *out, epi_pattern_summary *sum, PatmStats &st) {
  EPI_HIP(hipSetDevice(b->eng->device));
  hipStream_t s = pick_stream(b, stream);
  int64_t lmax = 0;
  EPI_TRY(pat_longest_row(b, s, &lmax));
  bool ranged = !b->h_stats.unsorted;
  std::vector<int64_t> pos_lo((size_t)nt), nwin((size_t)nt);
  for (int32_t t = 0; t < nt; t++) {
    if (t_start[t] < 0 || t_end[t] < 0) ranged = false;       // (pat_span compares unsigned)
    EPI_TRY(pat_window(t_start[t], t_end[t], lmax, reverse_offset, &pos_lo[(size_t)t], &nwin[(size_t)t]));
  }
  PatmCall c = patm_call(b, s, min_overlap, ctx, min_ctx_freq, clip, reverse_offset);
  c.t_rname = t_rname; c.t_start = t_start; c.t_end = t_end; c.pos_lo = pos_lo.data(); c.nwin = nwin.data();
  c.hlght = hlght; c.hlght_off = hlght_off; c.out = out; c.sum = sum; c.st = &st;
  PatmScratch w;
  std::vector<int64_t> h_rng;
  if (ranged) {
    EPI_TRY(patm_fetch_candidate_rows(c, w, nt, lmax, min_overlap, h_rng));
    ranged = !h_rng[(size_t)2 * nt];
  }
  if (!ranged) return patm_target_by_target(c, w, nt);
  c.rng = h_rng.data();
  // groups of consecutive targets whose pass-1 scratch (40 B per pair, 8 B per window position) fits the cap
  int rc = EPI_OK;
  for (int32_t ta = 0; ta < nt && rc == EPI_OK;) {
    int64_t bytes = 0;
    int32_t tb = ta;
    while (tb < nt) {
      const int64_t need = 40 * (h_rng[2 * (size_t)tb + 1] - h_rng[2 * (size_t)tb]) + 8 * nwin[(size_t)tb] + 128;
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
  int64_t lmax = 0, pos_lo = 0, nwin = 0;
  EPI_TRY(pat_longest_row(b, s, &lmax));
  EPI_TRY(pat_window(target_start, target_end, lmax, reverse_offset, &pos_lo, &nwin));
  const int64_t hlght_off[2] = {0, nhlght};
  PatmCall c = patm_call(b, s, min_overlap, ctx, min_ctx_freq, clip, reverse_offset);
  c.t_rname = &target_rname; c.t_start = &target_start; c.t_end = &target_end; c.pos_lo = &pos_lo; c.nwin = &nwin;
  c.hlght = hlght; c.hlght_off = hlght_off;
  PatmScratch w;
  return patm_all_rows(c, w, 0, out);
}

int epi_batch_extract_patterns_multi(epi_batch *b, int32_t ntargets, const int32_t *target_rname, const int32_t *target_start,
                                     const int32_t *target_end, int32_t min_overlap, const char *ctx, double min_ctx_freq, int32_t clip,
                                     int32_t reverse_offset, const int32_t *hlght, const int64_t *hlght_off, void *stream,
                                     epi_pattern_table *out) {
  if (ntargets > 0 && out) memset(out, 0, (size_t)ntargets * sizeof(*out));
  EPI_TRY(patm_check_args("epi_batch_extract_patterns_multi", b, ntargets, target_rname, target_start, target_end, ctx, hlght, hlght_off, out));
  b->pat.extract_groups = 0; b->pat.extract_pairs = 0; b->pat.extract_scratch = 0;
  if (ntargets == 0 || b->n == 0) return EPI_OK;
  PatmStats st;
  const int rc = patm_run(b, ntargets, target_rname, target_start, target_end, min_overlap, ctx, min_ctx_freq, clip, reverse_offset,
                          hlght, hlght_off, stream, out, nullptr, st);
  b->pat.extract_groups = st.groups; b->pat.extract_pairs = st.pairs; b->pat.extract_scratch = st.scratch;
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
  b->pat.summarise_groups = 0; b->pat.summarise_pairs = 0; b->pat.summarise_fallback = 0;
  if (ntargets == 0 || b->n == 0) return EPI_OK;
  PatmStats st;
  const int rc = patm_run(b, ntargets, target_rname, target_start, target_end, min_overlap, ctx, min_ctx_freq, clip, reverse_offset,
                          hlght, hlght_off, stream, nullptr, out, st);
  b->pat.summarise_groups = st.groups; b->pat.summarise_pairs = st.pairs; b->pat.summarise_fallback = st.fallback;
  if (rc != EPI_OK)
    for (int32_t t = 0; t < ntargets; t++) epi_pattern_summary_free(out + t);
  return rc;
}

int epi_batch_summarise_patterns_stats(epi_batch *b, int64_t *groups, int64_t *pairs, int64_t *fallback_targets) {
  if (!b) return fail(EPI_ERR_ARG, "epi_batch_summarise_patterns_stats: batch is NULL");
  if (groups) *groups = b->pat.summarise_groups;
  if (pairs) *pairs = b->pat.summarise_pairs;
  if (fallback_targets) *fallback_targets = b->pat.summarise_fallback;
  return EPI_OK;
}

int epi_batch_extract_patterns_multi_stats(epi_batch *b, int64_t *groups, int64_t *pairs, int64_t *scratch_bytes) {
  if (!b) return fail(EPI_ERR_ARG, "epi_batch_extract_patterns_multi_stats: batch is NULL");
  if (groups) *groups = b->pat.extract_groups;
  if (pairs) *pairs = b->pat.extract_pairs;
  if (scratch_bytes) *scratch_bytes = b->pat.extract_scratch;
  return EPI_OK;
}

}  // extern "C"
