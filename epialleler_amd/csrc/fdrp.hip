// FDRP report: the fraction of discordant read pairs (FDRP) and the mean normalised Hamming distance of read pairs (qFDRP)
// per cytosine, the two within-sample heterogeneity scores of the WSH package (Scherer et al. 2020; include/epihip.h,
// epi_batch_fdrp_report_dev, has the definitions).  No reference interface is replaced.  Sites, calls and kept rows are the
// heterogeneity report's (site_table.hpp); what is new is that rows are compared with each other, so the report first
// builds an index from a site to the rows that have a call there.
//
// Data path, all on the report's stream:
//  (a) the site table of the heterogeneity report: the un-thresholded CX report, split per strand (site_table).
//  (b) k_fdrp_mark: a group of G lanes (16, or 64 for long rows) takes a row as in k_het_count and leaves the row's first
//      site lo, its sites hi - lo, its calls and its words ceil((hi - lo) / 64); k_fdrp_sum_calls sums the calls of all rows
//      in 64 bits.  Two scans give every row its first pair and its first word; the two totals come back to the host
//      in the step's one synchronisation, and the number of calls goes through epi_fdrp_pair_bytes.
//  (c) k_fdrp_fill: the same walk.  The round's two ballots are ORed into the row's current words (bit j of a row = its site
//      lo + j: valid, methylated), and every call writes one (key = site, value = row) pair at the row's first pair + the
//      calls of the row in front of this one (the count of the earlier rounds + the lower lanes of the ballot): no place
//      comes from what an atomic returns.
//  (d) radix_sort.hip's stable LSD sort, in a SortPairs workspace, over the bytes that N - 1 occupies.  The pairs are written in
//      ascending row order, the sort is stable: the rows of site g are then a run in ascending row index.  k_fdrp_bounds
//      (a thread per pair) writes where the run of a site starts and ends; its length is the site's coverage.
//  (e) k_fdrp_pairs: a wavefront per site.  Lane j takes the j-th selected row and shifts the row's packed calls of the
//      window g - W .. g + W into one 64-bit word each (at most 63 bits; the window may straddle two words and may start in
//      front of the row).  The window's site mask (same sequence, within max_distance; one ballot of lanes 0 .. 2W over the
//      table keys, clipped to the strand's part) is ANDed in.  Then, for every a, the lanes b > a read row a's two words
//      (v_readlane: a is uniform), take two popcounts and count: npairs and ndiscordant per lane (summed over the wave at
//      the end), H[o] += h as LDS adds on 64 u32 counters of the wave.  Lane 0 adds H[o] / o in ascending o.
//  (f) k_fdrp_keep, site_rows, and at fetch k_fdrp_emit (a thread per CX row), as the heterogeneity report does.
// Every number that is reported is an integer count or is computed from integer counts by one thread in a fixed order: no
// launch shape or atomic order enters a result.
// State: epi_batch::sites (SiteReportState, common.hpp); frow, fbits, fpair and fsite are this report's and stay on the
// batch with the table: the site -> rows index.
#include "site_table.hpp"
#include "radix_sort.hpp"

namespace epi {

constexpr int kFdrpMaxW = 31, kFdrpMaxRows = 64;
constexpr int FDRP_WAVES = SITE_WG / 64;

struct FdrpRowArgs : SiteRows {
  uint32_t *row_lo, *row_ns, *row_nc, *row_nw;     // mark writes these ...
  unsigned long long *ncalls;
  const uint32_t *pair_off, *word_off;             // ... fill reads their scans
  uint64_t *valid, *meth;
  uint64_t *pkey;
  uint32_t *prow;
};

template <int G>
__global__ __launch_bounds__(SITE_WG) void k_fdrp_mark(FdrpRowArgs a) {
  constexpr int GPW = 64 / G;
  const uint32_t lane = threadIdx.x & 63u, sub = lane % G, grp = lane / G;
  const int64_t row = ((int64_t)blockIdx.x * (SITE_WG / 64) + (threadIdx.x >> 6)) * GPW + grp;
  const SiteRow<G> r(a, row, sub, grp);
  const uint32_t lo = r.lo, hi = r.hi;
  uint32_t nc = 0;
  for (uint32_t base = lo; __ballot(base < hi) != 0ull; base += G) {
    bool valid, meth;
    r.call(a, base + sub, valid, meth);
    nc += (uint32_t)__popcll(group_ballot<G>(valid, grp));
  }
  if (sub == 0 && row < a.n) {
    const uint32_t ns = hi - lo;
    a.row_lo[row] = lo; a.row_ns[row] = ns; a.row_nc[row] = nc; a.row_nw[row] = (ns + 63u) / 64u;
  }
}

// The calls of all rows in 64 bits (the scan over them is 32-bit: its total would wrap unnoticed).  A thread sums
// FDRP_SUM_ITEMS rows, a wave adds once.  (Not one add per wave of k_fdrp_mark: 2.5 M adds to one address for 10^7 rows
// serialise in L2 at 12 ns each, 30 ms; profiles/fdrp_report.txt.)
constexpr int FDRP_SUM_ITEMS = 16;
__global__ __launch_bounds__(SITE_WG) void k_fdrp_sum_calls(const uint32_t *__restrict__ row_nc, int64_t n, unsigned long long *__restrict__ ncalls) {
  const int64_t base = (int64_t)blockIdx.x * (SITE_WG * FDRP_SUM_ITEMS) + threadIdx.x;
  unsigned long long sum = 0;
#pragma unroll
  for (int i = 0; i < FDRP_SUM_ITEMS; i++) {
    const int64_t r = base + (int64_t)i * SITE_WG;
    if (r < n) sum += row_nc[r];
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) sum += __shfl_xor(sum, d, 64);
  if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(ncalls, sum);
}

template <int G>
__global__ __launch_bounds__(SITE_WG) void k_fdrp_fill(FdrpRowArgs a) {
  constexpr int GPW = 64 / G;
  const uint32_t lane = threadIdx.x & 63u, sub = lane % G, grp = lane / G;
  const int64_t row = ((int64_t)blockIdx.x * (SITE_WG / 64) + (threadIdx.x >> 6)) * GPW + grp;
  const SiteRow<G> r(a, row, sub, grp);
  const uint32_t lo = r.lo, hi = r.hi;
  const size_t p0 = row < a.n ? a.pair_off[row] : 0u, w0 = row < a.n ? a.word_off[row] : 0u;
  const unsigned long long below = (1ull << sub) - 1ull;
  uint32_t seen = 0;                                         // calls of the row in the rounds before this one
  unsigned long long accv = 0, accm = 0;                     // the word that is being filled
  for (uint32_t base = lo; __ballot(base < hi) != 0ull; base += G) {
    const uint32_t g = base + sub;
    bool valid, meth;
    r.call(a, g, valid, meth);
    const unsigned long long sv = group_ballot<G>(valid, grp), sm = group_ballot<G>(meth, grp);
    if (valid) {                                             // (g < hi: a site of this row)
      const size_t at = p0 + seen + (uint32_t)__popcll(sv & below);
      a.pkey[at] = g;
      a.prow[at] = (uint32_t)row;
    }
    seen += (uint32_t)__popcll(sv);
    if (base < hi) {
      const uint32_t rel = base - lo, sh = rel & 63u;        // (a multiple of G)
      accv |= sv << sh; accm |= sm << sh;
      if (sh + G == 64u || hi - base <= (uint32_t)G) {       // the word is full, or the row ends in it
        if (sub == 0) { a.valid[w0 + rel / 64u] = accv; a.meth[w0 + rel / 64u] = accm; }
        accv = 0; accm = 0;
      }
    }
  }
}

// sorted keys -> the run of every site that has one: [site_off, site_end); both are zero elsewhere (memset by the host)
__global__ __launch_bounds__(SITE_WG) void k_fdrp_bounds(const uint64_t *__restrict__ key, uint32_t n, uint32_t N,
                                                        uint32_t *__restrict__ site_off, uint32_t *__restrict__ site_end) {
  const uint32_t i = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = key[i];
  if (k >= N) return;
  if (i == 0 || key[i - 1] != k) site_off[k] = i;
  if (i == n - 1u || key[i + 1] != k) site_end[k] = i + 1u;
}

struct FdrpSite {                      // what the pair kernel leaves per site of the table
  uint32_t npairs, ndiscordant;
  double qnum;                         // sum over o of H[o] / o
};
static_assert(sizeof(FdrpSite) == 16, "FdrpSite layout");

struct FdrpPairArgs {
  const unsigned long long *key;       // the per-strand site table
  const uint32_t *n1;
  const uint32_t *site_off, *site_end, *rows;
  const uint32_t *row_lo, *row_ns, *word_off;
  const uint64_t *valid, *meth;
  FdrpSite *out;
  int64_t max_dist;
  uint32_t N;
  int32_t W, m, min_overlap;
};

// 64 bits of a row's packed array from its bit s on (s may be negative, above -64: zeros in front of the row); bits behind
// the row's last word are zero, as are those behind its last site inside that word
__device__ __forceinline__ uint64_t fdrp_bits(const uint64_t *__restrict__ w, uint32_t nw, int64_t s) {
  if (s < 0) return nw ? w[0] << (uint32_t)(-s) : 0ull;
  const uint64_t i = (uint64_t)s >> 6;
  const uint32_t b = (uint32_t)s & 63u;
  const uint64_t x = i < nw ? w[i] : 0ull, y = i + 1u < nw ? w[i + 1u] : 0ull;
  return b ? (x >> b) | (y << (64u - b)) : x;
}

__device__ __forceinline__ uint64_t wave_read_u64(uint64_t v, int l) {      // lane l's value; l is uniform
  const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)b << 32) | a;
}

__global__ __launch_bounds__(SITE_WG) void k_fdrp_pairs(FdrpPairArgs a) {
  __shared__ uint32_t s_H[FDRP_WAVES][64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  s_H[wave][lane] = 0;
  __syncthreads();
  const uint32_t g = blockIdx.x * (uint32_t)FDRP_WAVES + wave;
  const bool site = g < a.N;
  uint32_t c = 0, off = 0;
  if (site) { off = a.site_off[g]; c = a.site_end[g] - off; }
  const int nreads = __builtin_amdgcn_readfirstlane((int)(c < (uint32_t)a.m ? c : (uint32_t)a.m));
  const bool use = site && nreads >= 2;
  uint32_t np = 0, nd = 0;
  if (use) {
    const int W = a.W, nwin = 2 * W + 1;
    // the window's sites: those of g's sequence and strand, within max_dist of it
    const uint32_t n1 = *a.n1, s0 = g < n1 ? 0u : n1, s1 = g < n1 ? n1 : a.N;
    const unsigned long long kg = a.key[g];
    const int64_t gi = (int64_t)g - W + (int64_t)lane;
    bool ok = false;
    if ((int)lane < nwin && gi >= (int64_t)s0 && gi < (int64_t)s1) {
      const unsigned long long k = a.key[gi];
      const int64_t d = (int64_t)table_key_pos(k) - (int64_t)table_key_pos(kg);
      ok = (k >> 32) == (kg >> 32) && (a.max_dist == 0 || (d <= a.max_dist && -d <= a.max_dist));
    }
    const uint64_t mask = __ballot(ok);
    // lane j: the window of its row, bit t = site g - W + t
    uint64_t va = 0, ma = 0;
    if ((int)lane < nreads) {
      const uint32_t rank = c <= (uint32_t)a.m ? lane : (uint32_t)(((uint64_t)lane * c) / (uint32_t)a.m);
      const uint32_t row = a.rows[(size_t)off + rank];
      const uint32_t nw = (a.row_ns[row] + 63u) / 64u;
      const size_t w0 = a.word_off[row];
      const int64_t s = (int64_t)g - W - (int64_t)a.row_lo[row];          // >= -W: the row has a call at g
      va = fdrp_bits(a.valid + w0, nw, s) & mask;
      ma = fdrp_bits(a.meth + w0, nw, s) & va;
    }
    for (int x = 0; x + 1 < nreads; x++) {
      const uint64_t vx = wave_read_u64(va, x), mx = wave_read_u64(ma, x);
      if ((int)lane > x && (int)lane < nreads) {
        const uint64_t both = vx & va;
        const int o = __popcll(both), h = __popcll((mx ^ ma) & both);
        if (o >= a.min_overlap) {
          np++;
          if (h) { nd++; atomicAdd(&s_H[wave][o], (uint32_t)h); }      // o <= 63
        }
      }
    }
  }
  np = wave_sum_u32(np); nd = wave_sum_u32(nd);
  __syncthreads();
  if (site && lane == 0) {
    double q = 0.0;
    if (use)
      for (int o = 1; o <= 2 * a.W + 1; o++) q += (double)s_H[wave][o] / (double)o;     // ascending o
    FdrpSite r;
    r.npairs = np; r.ndiscordant = nd; r.qnum = q;
    a.out[g] = r;
  }
}

struct FdrpFinish : SiteView {
  uint32_t N;
  int32_t m;
  uint32_t min_reads;
  const uint32_t *site_off, *site_end;
  const FdrpSite *res;
};

__device__ __forceinline__ bool fdrp_site(const FdrpFinish &f, uint32_t i, uint32_t *g_out, uint32_t *cov, uint32_t *nreads) {
  const uint32_t g = site_ordinal(f.strand[i], i, f.rank[i], *f.n1);
  if (g >= f.N) return false;
  const uint32_t c = f.site_end[g] - f.site_off[g];
  *g_out = g; *cov = c; *nreads = c < (uint32_t)f.m ? c : (uint32_t)f.m;
  return true;
}

__global__ __launch_bounds__(SITE_WG) void k_fdrp_keep(FdrpFinish f, uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (i >= f.N) return;
  uint32_t g, c, nr;
  flag[i] = fdrp_site(f, i, &g, &c, &nr) && nr >= f.min_reads && f.res[g].npairs >= 1u ? 1u : 0u;
}

struct FdrpOut {
  int32_t *rname, *strand, *pos, *context, *coverage, *nreads, *npairs, *ndiscordant;
  double *fdrp, *qfdrp;
};

__global__ __launch_bounds__(SITE_WG) void k_fdrp_emit(FdrpFinish f, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ out_off,
                                                      FdrpOut o) {
  const uint32_t i = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (i >= f.N || !flag[i]) return;
  uint32_t g, c, nr;
  if (!fdrp_site(f, i, &g, &c, &nr)) return;
  const FdrpSite s = f.res[g];
  const uint32_t r = out_off[i];
  o.rname[r] = f.rname[i]; o.strand[r] = f.strand[i]; o.pos[r] = f.pos[i]; o.context[r] = f.context[i];
  o.coverage[r] = (int32_t)c; o.nreads[r] = (int32_t)nr; o.npairs[r] = (int32_t)s.npairs; o.ndiscordant[r] = (int32_t)s.ndiscordant;
  const double dn = (double)s.npairs;
  o.fdrp[r] = (double)s.ndiscordant / dn;
  o.qfdrp[r] = s.qnum / dn;
}

static void fdrp_finish_args(const epi_batch *b, FdrpFinish &f) {
  const SiteReportState &t = b->sites;
  f.N = site_view_args(b, f);
  f.m = t.fdrp.max_rows;
  f.min_reads = t.min_reads;
  f.site_off = t.fdrp.fsite.as<uint32_t>();
  f.site_end = f.site_off + f.N;
  f.res = t.counts.as<FdrpSite>();
}

// bytes of the two (key, row) buffers of ncalls pairs, or -1 when the sort's 32-bit indices cannot hold them
static int64_t fdrp_pair_bytes(int64_t ncalls) { return ncalls < 0 || ncalls >= (1LL << 32) ? -1 : (int64_t)SortPairs::pair_bytes((size_t)ncalls); }

static int fdrp_empty(epi_batch *b) { b->last_kind = KIND_FDRP; b->last_nrow = 0; b->sites.nsite = 0; return EPI_OK; }

static int fdrp_report(epi_batch *b, const char *ctx, int W, int m, int min_overlap, int32_t max_dist, double max_oo, int32_t min_reads,
                       hipStream_t s, int64_t *nrow_out) {
  const char *who = "epi_batch_fdrp_report_dev";
  SiteReportState &t = b->sites;
  // (a) the site table
  int64_t nsite = 0;
  EPI_TRY(site_cx_report(b, ctx, s, who, &nsite));
  t.nsite = nsite; t.fdrp.W = W; t.fdrp.max_rows = m; t.fdrp.min_overlap = min_overlap;
  t.min_reads = (uint32_t)(min_reads > 2 ? min_reads : 2);
  if (nsite == 0 || b->n == 0) return fdrp_empty(b);
  if (nsite >= (1LL << 31)) return fail(EPI_ERR_ARG, "%s: %lld sites, beyond 32-bit ordinals", who, (long long)nsite);
  if (b->nbytes / 64 + b->n >= (1LL << 32)) return fail(EPI_ERR_ARG, "%s: the rows' packed calls need 2^32 words or more", who);
  const size_t N = (size_t)nsite, n = (size_t)b->n;
  const int64_t nb_sites = ((int64_t)N + SITE_WG - 1) / SITE_WG, nb_waves = ((int64_t)N + FDRP_WAVES - 1) / FDRP_WAVES;
  bool wide = false;
  const int64_t nb_rows = site_count_blocks(b, &wide);
  EPI_TRY(check_grid(nb_rows, SITE_WG, "FDRP row kernels"));
  EPI_TRY(check_grid(nb_waves, SITE_WG, "FDRP pair kernel"));
  EPI_TRY(site_table(b, nsite, s));
  SiteScalars *sc = t.scalars();
  EPI_TRY(t.fdrp.frow.ensure(n * 6 * 4));

  // (b) what every row holds
  FdrpRowArgs a;
  site_rows_args(b, ctx_mask_of(ctx), max_oo, a);
  uint32_t *fr = t.fdrp.frow.as<uint32_t>();
  a.row_lo = fr; a.row_ns = fr + n; a.row_nc = fr + 2 * n; a.row_nw = fr + 3 * n;
  uint32_t *pair_off = fr + 4 * n, *word_off = fr + 5 * n;
  a.pair_off = pair_off; a.word_off = word_off;
  a.ncalls = &sc->ncalls;
  a.valid = a.meth = nullptr; a.pkey = nullptr; a.prow = nullptr;
  EPI_HIP(hipMemsetAsync(&sc->nwords, 0, 16, s));
  prof_begin("fdrp_mark", s);
  if (wide) hipLaunchKernelGGL((k_fdrp_mark<64>), dim3((unsigned)nb_rows), dim3(SITE_WG), 0, s, a);
  else hipLaunchKernelGGL((k_fdrp_mark<16>), dim3((unsigned)nb_rows), dim3(SITE_WG), 0, s, a);
  hipLaunchKernelGGL(k_fdrp_sum_calls, dim3((unsigned)((n + SITE_WG * FDRP_SUM_ITEMS - 1) / (SITE_WG * FDRP_SUM_ITEMS))), dim3(SITE_WG), 0, s,
                     a.row_nc, (int64_t)n, a.ncalls);
  prof_end("fdrp_mark", s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(scan_exclusive_u32(a.row_nc, pair_off, (int64_t)n, nullptr, b->scan_tmp, s));
  EPI_TRY(scan_exclusive_u32(a.row_nw, word_off, (int64_t)n, &sc->nwords, b->scan_tmp, s));
  struct { uint32_t nwords, unused; unsigned long long ncalls; } h = {0, 0, 0};
  EPI_TRY(read_scalars(b, s, &sc->nwords, 16, &h));
  if (h.ncalls == 0) return fdrp_empty(b);
  const int64_t pbytes = h.ncalls >> 32 ? -1 : fdrp_pair_bytes((int64_t)h.ncalls);
  if (pbytes < 0)
    return fail(EPI_ERR_ARG, "%s: %llu calls, the site -> rows index holds fewer than 2^32 pairs", who, h.ncalls);
  const size_t nc = (size_t)h.ncalls, nw = h.nwords;
  const int64_t nb_pairs = ((int64_t)nc + SITE_WG - 1) / SITE_WG;
  EPI_TRY(check_grid(nb_pairs, SITE_WG, "FDRP index kernels"));

  // (c) the packed calls and the (site, row) pairs
  EPI_TRY(t.fdrp.fpair.ensure(SortPairs::bytes(nc)));
  EPI_TRY(t.fdrp.fbits.ensure(nw * 16));
  EPI_TRY(t.fdrp.fsite.ensure(N * 8));
  EPI_TRY(t.counts.ensure(N * sizeof(FdrpSite)));
  EPI_TRY(t.out.ensure(N * 4));
  SortPairs sort(t.fdrp.fpair.p, nc);
  a.valid = t.fdrp.fbits.as<uint64_t>(); a.meth = a.valid + nw;
  a.pkey = sort.keys_in(); a.prow = sort.vals_in();
  prof_begin("fdrp_fill", s);
  if (wide) hipLaunchKernelGGL((k_fdrp_fill<64>), dim3((unsigned)nb_rows), dim3(SITE_WG), 0, s, a);
  else hipLaunchKernelGGL((k_fdrp_fill<16>), dim3((unsigned)nb_rows), dim3(SITE_WG), 0, s, a);
  prof_end("fdrp_fill", s);
  EPI_HIP(hipGetLastError());

  // (d) the rows of a site, in ascending row index
  uint32_t bytes = 0;
  for (int d = 0; d < 4; d++) if ((N - 1) >> (8 * d)) bytes |= 1u << d;
  EPI_TRY(sort.sort(bytes, b->scan_tmp, s));
  uint32_t *site_off = t.fdrp.fsite.as<uint32_t>(), *site_end = site_off + N;
  EPI_HIP(hipMemsetAsync(site_off, 0, N * 8, s));
  prof_begin("fdrp_bounds", s);
  hipLaunchKernelGGL(k_fdrp_bounds, dim3((unsigned)nb_pairs), dim3(SITE_WG), 0, s, sort.keys(), (uint32_t)nc, (uint32_t)N, site_off, site_end);
  prof_end("fdrp_bounds", s);

  // (e) the pairs of every site
  FdrpPairArgs p;
  p.key = t.key.as<unsigned long long>(); p.n1 = &sc->nplus; p.N = (uint32_t)N;
  p.site_off = site_off; p.site_end = site_end; p.rows = sort.vals();
  p.row_lo = a.row_lo; p.row_ns = a.row_ns; p.word_off = word_off;
  p.valid = a.valid; p.meth = a.meth;
  p.out = t.counts.as<FdrpSite>();
  p.max_dist = max_dist; p.W = W; p.m = m; p.min_overlap = min_overlap;
  prof_begin("fdrp_pairs", s);
  hipLaunchKernelGGL(k_fdrp_pairs, dim3((unsigned)nb_waves), dim3(SITE_WG), 0, s, p);
  prof_end("fdrp_pairs", s);
  EPI_HIP(hipGetLastError());

  // (f) which sites are reported, and where
  FdrpFinish f;
  fdrp_finish_args(b, f);
  uint32_t *flag = t.flag.as<uint32_t>();
  hipLaunchKernelGGL(k_fdrp_keep, dim3((unsigned)nb_sites), dim3(SITE_WG), 0, s, f, flag);
  EPI_HIP(hipGetLastError());
  EPI_TRY(site_rows(b, flag, (int64_t)N, t.out.as<uint32_t>(), &sc->nrow, s, nrow_out));
  b->last_kind = KIND_FDRP;
  b->last_nrow = *nrow_out;
  return EPI_OK;
}

}  // namespace epi

using namespace epi;

extern "C" {

int epi_fdrp_pair_bytes(int64_t ncalls, int64_t *bytes_out) {
  if (!bytes_out) return fail(EPI_ERR_ARG, "epi_fdrp_pair_bytes: NULL argument");
  *bytes_out = 0;
  const int64_t bytes = fdrp_pair_bytes(ncalls);
  if (bytes < 0) return fail(EPI_ERR_ARG, "epi_fdrp_pair_bytes: %lld calls, the pair list holds 0 to 2^32 - 1", (long long)ncalls);
  *bytes_out = bytes;
  return EPI_OK;
}

int epi_batch_fdrp_report_dev(epi_batch *b, const char *ctx, int flank_sites, int max_reads, int min_overlap, int32_t max_distance,
                              double max_ooctx_meth_frac, int32_t min_reads, void *stream, int64_t *nrow_out) {
  const char *who = "epi_batch_fdrp_report_dev";
  if (!b || !ctx || !nrow_out) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  *nrow_out = 0;
  if (flank_sites < 0 || flank_sites > kFdrpMaxW) return fail(EPI_ERR_ARG, "%s: flank_sites = %d, a window holds 0 to %d sites on either side", who, flank_sites, kFdrpMaxW);
  if (max_reads < 2 || max_reads > kFdrpMaxRows) return fail(EPI_ERR_ARG, "%s: max_reads = %d, 2 to %d reads are compared per site", who, max_reads, kFdrpMaxRows);
  if (min_overlap < 1 || min_overlap > 2 * flank_sites + 1)
    return fail(EPI_ERR_ARG, "%s: min_overlap = %d, 1 to %d (the window's sites)", who, min_overlap, 2 * flank_sites + 1);
  if (max_distance < 0) return fail(EPI_ERR_ARG, "%s: negative max_distance", who);
  b->last_kind = KIND_NONE;
  EPI_HIP(hipSetDevice(b->eng->device));
  return fdrp_report(b, ctx, flank_sites, max_reads, min_overlap, max_distance, max_ooctx_meth_frac, min_reads, pick_stream(b, stream), nrow_out);
}

int epi_batch_fdrp_fetch_dev(epi_batch *b, int32_t *const d_icols[8], double *const d_dcols[2], void *stream) {
  hipStream_t s = nullptr;
  int64_t nrow = 0;
  EPI_TRY(site_fetch_begin("epi_batch_fdrp_fetch_dev", b, KIND_FDRP, "FDRP report", false, d_icols, 8, d_dcols, 2, stream, &s, &nrow));
  if (nrow == 0) return EPI_OK;
  FdrpFinish f;
  fdrp_finish_args(b, f);
  FdrpOut o;
  o.rname = d_icols[0]; o.strand = d_icols[1]; o.pos = d_icols[2]; o.context = d_icols[3]; o.coverage = d_icols[4];
  o.nreads = d_icols[5]; o.npairs = d_icols[6]; o.ndiscordant = d_icols[7];
  o.fdrp = d_dcols[0]; o.qfdrp = d_dcols[1];
  const unsigned nb = (unsigned)(((int64_t)f.N + SITE_WG - 1) / SITE_WG);
  prof_begin("fdrp_emit", s);
  hipLaunchKernelGGL(k_fdrp_emit, dim3(nb), dim3(SITE_WG), 0, s, f, b->sites.flag.as<uint32_t>(), b->sites.out.as<uint32_t>(), o);
  prof_end("fdrp_emit", s);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

}  // extern "C"
