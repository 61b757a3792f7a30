// Linkage report: co-methylation of pairs of neighbouring sites over the reads that cover both -- the 2 x 2 table of
// every pair (s_j, s_{j+d}), d = 1 .. D, its covariance, r^2 and D' -- and the methylation haplotype blocks that follow
// from r^2 (Guo et al. 2017; include/epihip.h, epi_batch_linkage_report_dev, has the definitions).  No reference interface
// is replaced.  The data path is the heterogeneity report's (heterogeneity.hip; the shared parts are in site_table.hpp):
//  (a) the same site table: the un-thresholded CX report, split per strand, 64-bit keys and context codes.
//  (b) k_link_count: a group of G lanes (16, or 64 for long rows) takes a row: the read rule, the (G + 1)-ary search for the
//      row's site range [lo, hi), then G sites per round with the two ballots.  The lane at site g with a call looks back
//      d = 1 .. D in the round's valid / methylated masks (the previous round's last D bits carried over for the first
//      lanes; D <= 16 <= G: one previous round suffices) and adds 1 to counts[((g - d) D + d - 1) 4 + p] for every called
//      site it finds, p = meth(s_{g-d}) + 2 meth(s_g).  What lies between the two sites does not matter.
//  (c) k_link_keep (a thread per CX row and d): n, min_reads, the distance cap -> a flag; util.hip's scan (site_rows);
//      k_link_emit (at fetch) writes the pair's row and metrics.
//  (d) blocks, from the counters (nothing is read back from the emitted table): k_link_back (a thread per site) counts
//      the leading linked pairs behind a site; k_link_blocks (a thread per run head: a strand's first site or a site with
//      back = 0) walks greedily to the next run head and leaves every block's length and mean r^2 at its first site;
//      k_link_block_flag, the scan and k_link_block_emit bring them into CX row order.
// The site table, the counters [site][D][4], the keep flags and output rows [site][D] and the blocks' buffers are those of
// epi_batch::sites (SiteReportState, common.hpp), where every report of this family keeps its state.
// Every metric is computed by one thread from the four integers of its pair: no launch shape enters a result.
//
// Contention.  As in k_het_count the four rows of a wave of 16-lane groups walk the same sites when they start together
// (a deep amplicon).  Once per round every lane reads the base site and the two look-back windows of the lanes
// sub + 16 m of the other groups; for each d the lanes that hold the same counter then add once, the lowest of them the
// set's size.  Nine cross-lane reads per round whatever D is.
#include "site_table.hpp"

namespace epi {

constexpr int kLinkMaxD = 16;
constexpr int64_t kLinkCountsCap = 4LL << 30;         // bytes of counters (nsites * D * 16) a report may allocate
static_assert(kLinkMaxD <= 16, "k_link_count<16> carries the bits of one previous round of 16 sites");

struct LinkArgs : SiteRows {
  int32_t D;
  uint32_t *counts;                   // [N][D][4]: pair (g, d) at (g D + d - 1) 4, bins n_uu, n_mu, n_um, n_mm
};

// bytes of counters for nsites sites and D neighbours, or -1 when a report refuses them
static int64_t link_counter_bytes(int64_t nsites, int D) {
  if (nsites < 0 || D < 1 || D > kLinkMaxD || nsites >= (1LL << 31)) return -1;
  const int64_t bytes = nsites * D * 16;
  return bytes > kLinkCountsCap ? -1 : bytes;
}

template <int G>
__global__ __launch_bounds__(SITE_WG) void k_link_count(LinkArgs a) {
  static_assert(G >= kLinkMaxD, "the look-back reaches one previous round");
  constexpr int GPW = 64 / G;                                // groups per wave
  const uint32_t lane = threadIdx.x & 63u, sub = lane % G, grp = lane / G;
  const int64_t row = ((int64_t)blockIdx.x * (SITE_WG / 64) + (threadIdx.x >> 6)) * GPW + grp;
  const SiteRow<G> r(a, row, sub, grp);
  const uint32_t lo = r.lo, hi = r.hi;

  const int D = a.D;
  const uint32_t dmask = (1u << D) - 1u;
  uint32_t carry_v = 0, carry_m = 0;                         // the D sites in front of this round, oldest at bit 0
  for (uint32_t base = lo; __ballot(base < hi) != 0ull; base += G) {
    const uint32_t g = base + sub;
    bool valid, meth;
    r.call(a, g, valid, meth);
    const unsigned long long sv = group_ballot<G>(valid, grp), sm = group_ballot<G>(meth, grp);
    // the D + 1 sites that end at this lane's: bit D is its own, bit D - d the site d behind it
    uint32_t wv, wm;
    if ((int)sub >= D) { wv = (uint32_t)(sv >> (sub - D)); wm = (uint32_t)(sm >> (sub - D)); }
    else { wv = (uint32_t)(sv << (D - sub)) | (carry_v >> sub); wm = (uint32_t)(sm << (D - sub)) | (carry_m >> sub); }
    wv = valid ? wv & (dmask | (1u << D)) : 0u;              // no call here: no pair ends here
    wm &= wv;
    // a site d behind a called one is a site of the row: calls come from [lo, hi) only, the carry starts empty
    if constexpr (G < 64) {
      uint32_t ob[GPW], ov[GPW], om[GPW];
      bool obelow[GPW];
#pragma unroll
      for (int m = 1; m < GPW; m++) {
        const int src = (int)((lane + m * G) & 63u);
        ob[m] = __shfl(base, src, 64); ov[m] = __shfl(wv, src, 64); om[m] = __shfl(wm, src, 64);
        obelow[m] = (uint32_t)src < lane;
        if (ob[m] != base) ov[m] = 0u;                       // another site: never the same counter
      }
      for (int d = 1; d <= D; d++) {
        const uint32_t bit = 1u << (D - d);
        if (!__ballot((wv & bit) != 0u)) continue;
        const uint32_t pm = wm & (bit | (1u << D));          // the pair's two calls
        uint32_t same = 1u;
        bool first = true;
#pragma unroll
        for (int m = 1; m < GPW; m++)
          if ((ov[m] & bit) && (om[m] & (bit | (1u << D))) == pm) { same++; if (obelow[m]) first = false; }
        if ((wv & bit) && first) {
          const uint32_t p = ((pm & bit) ? 1u : 0u) | ((pm >> D) << 1);
          atomicAdd(&a.counts[(((size_t)(g - (uint32_t)d) * (uint32_t)D + (uint32_t)(d - 1)) << 2) + p], same);
        }
      }
    } else {
      for (int d = 1; d <= D; d++) {
        const uint32_t bit = 1u << (D - d);
        if (wv & bit) {
          const uint32_t p = ((wm & bit) ? 1u : 0u) | ((wm >> D) << 1);
          atomicAdd(&a.counts[(((size_t)(g - (uint32_t)d) * (uint32_t)D + (uint32_t)(d - 1)) << 2) + p], 1u);
        }
      }
    }
    carry_v = (uint32_t)(sv >> (G - D)) & dmask;
    carry_m = (uint32_t)(sm >> (G - D)) & dmask;
  }
}

struct LinkFinish : SiteView {
  uint32_t N;
  int32_t D;
  uint32_t min_reads;
  int64_t max_dist;
};

struct LinkPair {
  uint32_t uu, mu, um, mm;
  uint64_t n;
  int32_t pos, pos2;
  bool reported;                       // n >= min_reads and within the distance cap
};

// pair (g, d) by the ordinal of its first site: false when fewer than d sites follow g on its (rname, strand)
__device__ __forceinline__ bool link_pair(const LinkFinish &f, uint32_t g, int d, LinkPair &q) {
  const uint32_t n1 = *f.n1;
  const uint32_t seg_end = g < n1 ? n1 : f.N, g2 = g + (uint32_t)d;
  if (g2 >= seg_end) return false;
  const unsigned long long k1 = f.key[g], k2 = f.key[g2];
  if ((k1 >> 32) != (k2 >> 32)) return false;
  const uint32_t *c = f.counts + (((size_t)g * (uint32_t)f.D + (uint32_t)(d - 1)) << 2);
  q.uu = c[0]; q.mu = c[1]; q.um = c[2]; q.mm = c[3];
  q.n = (uint64_t)q.uu + q.mu + q.um + q.mm;
  q.pos = table_key_pos(k1); q.pos2 = table_key_pos(k2);
  q.reported = q.n >= (uint64_t)f.min_reads && (f.max_dist == 0 || (int64_t)q.pos2 - (int64_t)q.pos <= f.max_dist);
  return true;
}

// cov, r^2 and D' of a 2 x 2 table (include/epihip.h): r^2 and D' are NaN when a margin is 0
__device__ __forceinline__ void link_metrics(const LinkPair &q, double *cov, double *r2, double *dprime) {
  const int64_t mm = q.mm, mu = q.mu, um = q.um, uu = q.uu;
  const int64_t A = mm + mu, a = um + uu, B = mm + um, b = mu + uu;
  const int64_t num = mm * uu - mu * um;                     // |num| <= n^2 / 4 < 2^62
  const double dn = (double)q.n, dnum = (double)num;
  *cov = dnum / (dn * dn);
  if (A == 0 || a == 0 || B == 0 || b == 0) {
    *r2 = __longlong_as_double(0x7FF8000000000000LL);
    *dprime = *r2;
    return;
  }
  *r2 = (dnum * dnum) / ((((double)A * (double)a) * (double)B) * (double)b);
  if (num > 0) { const int64_t x = A * b, y = a * B; *dprime = dnum / (double)(x < y ? x : y); }
  else if (num < 0) { const int64_t x = A * B, y = a * b; *dprime = dnum / (double)(x < y ? x : y); }
  else *dprime = 0.0;
}

__global__ __launch_bounds__(SITE_WG) void k_link_keep(LinkFinish f, uint32_t *__restrict__ flag) {
  const uint32_t t = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  const uint32_t D = (uint32_t)f.D;
  if (t >= f.N * D) return;                                  // N D <= 2^28 (the counter cap)
  const uint32_t i = t / D, d = t % D + 1u;
  LinkPair q;
  const bool have = link_pair(f, site_ordinal(f.strand[i], i, f.rank[i], *f.n1), (int)d, q);
  flag[t] = have && q.reported ? 1u : 0u;
}

struct LinkOut {
  int32_t *rname, *strand, *pos, *pos2, *context, *neighbour, *nreads, *uu, *mu, *um, *mm;
  double *cov, *r2, *dprime;
};

__global__ __launch_bounds__(SITE_WG) void k_link_emit(LinkFinish f, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ out_off,
                                                      LinkOut o) {
  const uint32_t t = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  const uint32_t D = (uint32_t)f.D;
  if (t >= f.N * D || !flag[t]) return;
  const uint32_t i = t / D, d = t % D + 1u;
  LinkPair q;
  if (!link_pair(f, site_ordinal(f.strand[i], i, f.rank[i], *f.n1), (int)d, q)) return;
  const uint32_t r = out_off[t];
  o.rname[r] = f.rname[i]; o.strand[r] = f.strand[i]; o.pos[r] = f.pos[i]; o.pos2[r] = q.pos2; o.context[r] = f.context[i];
  o.neighbour[r] = (int32_t)d; o.nreads[r] = (int32_t)q.n;
  o.uu[r] = (int32_t)q.uu; o.mu[r] = (int32_t)q.mu; o.um[r] = (int32_t)q.um; o.mm[r] = (int32_t)q.mm;
  double cov, r2, dp;
  link_metrics(q, &cov, &r2, &dp);
  o.cov[r] = cov; o.r2[r] = r2; o.dprime[r] = dp;
}

// ---- blocks ----------------------------------------------------------------------------------------------------------------

// pair (g, d) is linked: reported and r^2 >= min_r2 (NaN: not linked)
__device__ __forceinline__ bool link_linked(const LinkFinish &f, uint32_t g, int d, double min_r2, double *r2_out) {
  LinkPair q;
  if (!link_pair(f, g, d, q) || !q.reported) return false;
  double cov, r2, dp;
  link_metrics(q, &cov, &r2, &dp);
  *r2_out = r2;
  return r2 >= min_r2;
}

// first ordinal of the strand part that holds e
__device__ __forceinline__ uint32_t link_seg_start(const LinkFinish &f, uint32_t e) { const uint32_t n1 = *f.n1; return e < n1 ? 0u : n1; }

// back[e]: the leading d = 1, 2, ... for which pair (e - d, d) is linked (a pair never leaves e's sequence and strand)
__global__ __launch_bounds__(SITE_WG) void k_link_back(LinkFinish f, double min_r2, uint8_t *__restrict__ back) {
  const uint32_t e = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (e >= f.N) return;
  const uint32_t s0 = link_seg_start(f, e);
  int t = 0;
  double r2;
  while (t < f.D && e - s0 > (uint32_t)t && link_linked(f, e - (uint32_t)(t + 1), t + 1, min_r2, &r2)) t++;
  back[e] = (uint8_t)t;
}

// is ordinal e the first site of its (rname, strand)?
__device__ __forceinline__ bool link_strand_head(const LinkFinish &f, uint32_t e) {
  return e == link_seg_start(f, e) || (f.key[e - 1] >> 32) != (f.key[e] >> 32);
}

// A thread per run head walks its run [e, next run head): blocks are built greedily, a block's length and the mean of its
// adjacent r^2 values (summed in ascending site order) go to its first site.  blen is zero elsewhere (memset by the host).
__global__ __launch_bounds__(SITE_WG) void k_link_blocks(LinkFinish f, double min_r2, int32_t min_sites, const uint8_t *__restrict__ back,
                                                        uint32_t *__restrict__ blen, double *__restrict__ bmean) {
  const uint32_t h = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (h >= f.N) return;
  if (back[h] != 0 && !link_strand_head(f, h)) return;
  const uint32_t n1 = *f.n1, seg_end = h < n1 ? n1 : f.N;
  uint32_t s = h;
  for (;;) {
    uint32_t e = s;
    double sum = 0.0;
    // extend while e + 1 is on the strand (a strand's first site has back = 0) and is linked to all it must be
    while (e + 1u < seg_end) {
      const uint32_t need = e + 1u - s < (uint32_t)f.D ? e + 1u - s : (uint32_t)f.D;
      if (back[e + 1u] < need) break;                         // (need >= 1: back = 0 ends the run)
      double r2 = 0.0;
      link_linked(f, e, 1, min_r2, &r2);                      // linked: back[e + 1] >= 1
      sum += r2;
      e++;
    }
    const uint32_t len = e - s + 1u;
    if (len >= (uint32_t)min_sites) { blen[s] = len; bmean[s] = sum / (double)(len - 1u); }
    s = e + 1u;
    if (s >= seg_end || back[s] == 0) return;                 // the next run head's thread goes on from here
  }
}

__global__ __launch_bounds__(SITE_WG) void k_link_block_flag(LinkFinish f, const uint32_t *__restrict__ blen, uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (i >= f.N) return;
  flag[i] = blen[site_ordinal(f.strand[i], i, f.rank[i], *f.n1)] ? 1u : 0u;
}

struct LinkBlockOut {
  int32_t *rname, *strand, *start, *end, *nsites;
  double *mean_r2;
};

__global__ __launch_bounds__(SITE_WG) void k_link_block_emit(LinkFinish f, const uint32_t *__restrict__ blen, const double *__restrict__ bmean,
                                                            const uint32_t *__restrict__ flag, const uint32_t *__restrict__ out_off,
                                                            LinkBlockOut o) {
  const uint32_t i = blockIdx.x * (uint32_t)SITE_WG + threadIdx.x;
  if (i >= f.N || !flag[i]) return;
  const uint32_t g = site_ordinal(f.strand[i], i, f.rank[i], *f.n1), len = blen[g], r = out_off[i];
  o.rname[r] = f.rname[i]; o.strand[r] = f.strand[i]; o.start[r] = f.pos[i];
  o.end[r] = table_key_pos(f.key[g + len - 1u]);               // the walk stayed inside the strand part
  o.nsites[r] = (int32_t)len;
  o.mean_r2[r] = bmean[g];
}

static void link_finish_args(const epi_batch *b, LinkFinish &f) {
  f.N = site_view_args(b, f);
  f.D = b->sites.link.D;
  f.min_reads = b->sites.min_reads;
  f.max_dist = b->sites.link.max_dist;
}

static int link_report(epi_batch *b, const char *ctx, int D, int32_t max_dist, double max_oo, int32_t min_reads, hipStream_t s,
                       int64_t *nrow_out) {
  SiteReportState &t = b->sites;
  // (a) the site table
  int64_t nsite = 0;
  EPI_TRY(site_cx_report(b, ctx, s, "epi_batch_linkage_report_dev", &nsite));
  t.nsite = nsite; t.link.D = D;
  t.min_reads = (uint32_t)(min_reads > 1 ? min_reads : 1);
  t.link.max_dist = max_dist;
  t.link.blocks = false; t.link.nblock = 0;
  if (nsite < 2) { b->last_kind = KIND_LINK; b->last_nrow = 0; t.nsite = 0; return EPI_OK; }
  const int64_t cbytes = link_counter_bytes(nsite, D);
  if (cbytes < 0)
    return fail(EPI_ERR_ARG, "epi_batch_linkage_report_dev: %lld sites x %d neighbours need %lld bytes of counters, above the cap of %lld",
                (long long)nsite, D, (long long)(nsite * D * 16), (long long)kLinkCountsCap);
  const size_t N = (size_t)nsite, ND = N * (size_t)D;
  const int64_t nb_pairs = ((int64_t)ND + SITE_WG - 1) / SITE_WG;
  bool wide = false;
  const int64_t nb_rows = site_count_blocks(b, &wide);
  EPI_TRY(check_grid(nb_pairs, SITE_WG, "linkage pair kernels"));
  EPI_TRY(check_grid(nb_rows, SITE_WG, "linkage counting kernel"));
  EPI_TRY(site_table(b, nsite, s));
  EPI_TRY(t.counts.ensure((size_t)cbytes));
  EPI_TRY(t.flag.ensure(ND * 4));                            // (the site table is done with its N words)
  EPI_TRY(t.out.ensure(ND * 4));
  uint32_t *flag = t.flag.as<uint32_t>();

  // (b) the 2 x 2 tables
  EPI_HIP(hipMemsetAsync(t.counts.p, 0, (size_t)cbytes, s));
  LinkArgs a;
  site_rows_args(b, ctx_mask_of(ctx), max_oo, a);
  a.D = D;
  a.counts = t.counts.as<uint32_t>();
  prof_begin("link_count", s);
  if (wide) hipLaunchKernelGGL((k_link_count<64>), dim3((unsigned)nb_rows), dim3(SITE_WG), 0, s, a);
  else hipLaunchKernelGGL((k_link_count<16>), dim3((unsigned)nb_rows), dim3(SITE_WG), 0, s, a);
  prof_end("link_count", s);
  EPI_HIP(hipGetLastError());

  // (c) which pairs are reported, and where
  LinkFinish f;
  link_finish_args(b, f);
  hipLaunchKernelGGL(k_link_keep, dim3((unsigned)nb_pairs), dim3(SITE_WG), 0, s, f, flag);
  EPI_HIP(hipGetLastError());
  EPI_TRY(site_rows(b, flag, (int64_t)ND, t.out.as<uint32_t>(), &t.scalars()->nrow, s, nrow_out));
  b->last_kind = KIND_LINK;
  b->last_nrow = *nrow_out;
  return EPI_OK;
}

// (d) the blocks of the last linkage report on b
static int link_blocks(epi_batch *b, double min_r2, int32_t min_sites, hipStream_t s, int64_t *nblock_out) {
  SiteReportState &t = b->sites;
  t.link.blocks = false; t.link.nblock = 0;
  const size_t N = (size_t)t.nsite;
  if (N == 0) { t.link.blocks = true; return EPI_OK; }
  const unsigned nb = (unsigned)(((int64_t)N + SITE_WG - 1) / SITE_WG);
  EPI_TRY(t.link.back.ensure(N));
  EPI_TRY(t.link.blen.ensure(N * 4));
  EPI_TRY(t.link.bmean.ensure(N * 8));
  EPI_TRY(t.link.bflag.ensure(N * 4));
  EPI_TRY(t.link.bout.ensure(N * 4));
  LinkFinish f;
  link_finish_args(b, f);
  uint32_t *blen = t.link.blen.as<uint32_t>(), *flag = t.link.bflag.as<uint32_t>();
  EPI_HIP(hipMemsetAsync(blen, 0, N * 4, s));
  hipLaunchKernelGGL(k_link_back, dim3(nb), dim3(SITE_WG), 0, s, f, min_r2, t.link.back.as<uint8_t>());
  hipLaunchKernelGGL(k_link_blocks, dim3(nb), dim3(SITE_WG), 0, s, f, min_r2, min_sites, t.link.back.as<uint8_t>(), blen, t.link.bmean.as<double>());
  hipLaunchKernelGGL(k_link_block_flag, dim3(nb), dim3(SITE_WG), 0, s, f, blen, flag);
  EPI_HIP(hipGetLastError());
  EPI_TRY(site_rows(b, flag, (int64_t)N, t.link.bout.as<uint32_t>(), &t.scalars()->nblock, s, nblock_out));
  t.link.blocks = true;
  t.link.nblock = *nblock_out;
  return EPI_OK;
}

}  // namespace epi

using namespace epi;

extern "C" {

int epi_linkage_counter_bytes(int64_t nsites, int max_neighbours, int64_t *bytes_out) {
  if (!bytes_out) return fail(EPI_ERR_ARG, "epi_linkage_counter_bytes: NULL argument");
  *bytes_out = 0;
  if (nsites < 0 || max_neighbours < 1 || max_neighbours > kLinkMaxD)
    return fail(EPI_ERR_ARG, "epi_linkage_counter_bytes: %lld sites, %d neighbours (1 to %d)", (long long)nsites, max_neighbours, kLinkMaxD);
  const int64_t bytes = link_counter_bytes(nsites, max_neighbours);
  if (bytes < 0)
    return fail(EPI_ERR_ARG, "epi_linkage_counter_bytes: %lld sites x %d neighbours need more than %lld bytes of counters",
                (long long)nsites, max_neighbours, (long long)kLinkCountsCap);
  *bytes_out = bytes;
  return EPI_OK;
}

int epi_batch_linkage_report_dev(epi_batch *b, const char *ctx, int max_neighbours, int32_t max_distance,
                                 double max_ooctx_meth_frac, int32_t min_reads, void *stream, int64_t *nrow_out) {
  if (!b || !ctx || !nrow_out) return fail(EPI_ERR_ARG, "epi_batch_linkage_report_dev: NULL argument");
  *nrow_out = 0;
  if (max_neighbours < 1 || max_neighbours > kLinkMaxD)
    return fail(EPI_ERR_ARG, "epi_batch_linkage_report_dev: max_neighbours = %d, a site is paired with 1 to %d neighbours", max_neighbours, kLinkMaxD);
  if (max_distance < 0) return fail(EPI_ERR_ARG, "epi_batch_linkage_report_dev: negative max_distance");
  b->last_kind = KIND_NONE;
  EPI_HIP(hipSetDevice(b->eng->device));
  return link_report(b, ctx, max_neighbours, max_distance, max_ooctx_meth_frac, min_reads, pick_stream(b, stream), nrow_out);
}

int epi_batch_linkage_fetch_dev(epi_batch *b, int32_t *const d_icols[11], double *const d_dcols[3], void *stream) {
  hipStream_t s = nullptr;
  int64_t nrow = 0;
  EPI_TRY(site_fetch_begin("epi_batch_linkage_fetch_dev", b, KIND_LINK, "linkage report", false, d_icols, 11, d_dcols, 3, stream, &s, &nrow));
  if (nrow == 0) return EPI_OK;
  LinkFinish f;
  link_finish_args(b, f);
  LinkOut o;
  o.rname = d_icols[0]; o.strand = d_icols[1]; o.pos = d_icols[2]; o.pos2 = d_icols[3]; o.context = d_icols[4];
  o.neighbour = d_icols[5]; o.nreads = d_icols[6]; o.uu = d_icols[7]; o.mu = d_icols[8]; o.um = d_icols[9]; o.mm = d_icols[10];
  o.cov = d_dcols[0]; o.r2 = d_dcols[1]; o.dprime = d_dcols[2];
  const unsigned nb = (unsigned)(((int64_t)f.N * f.D + SITE_WG - 1) / SITE_WG);
  hipLaunchKernelGGL(k_link_emit, dim3(nb), dim3(SITE_WG), 0, s, f, b->sites.flag.as<uint32_t>(), b->sites.out.as<uint32_t>(), o);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

int epi_batch_linkage_blocks_dev(epi_batch *b, double min_r2, int32_t min_sites, void *stream, int64_t *nblock_out) {
  if (!b || !nblock_out) return fail(EPI_ERR_ARG, "epi_batch_linkage_blocks_dev: NULL argument");
  *nblock_out = 0;
  if (b->last_kind != KIND_LINK) return fail(EPI_ERR_STATE, "epi_batch_linkage_blocks_dev: no finished linkage report on this batch");
  if (!(min_r2 >= 0.0 && min_r2 <= 1.0)) return fail(EPI_ERR_ARG, "epi_batch_linkage_blocks_dev: min_r2 outside [0, 1]");
  if (min_sites < 2) return fail(EPI_ERR_ARG, "epi_batch_linkage_blocks_dev: min_sites = %d, a block holds at least 2 sites", (int)min_sites);
  EPI_HIP(hipSetDevice(b->eng->device));
  return link_blocks(b, min_r2, min_sites, pick_stream(b, stream), nblock_out);
}

int epi_batch_linkage_blocks_fetch_dev(epi_batch *b, int32_t *const d_icols[5], double *const d_dcols[1], void *stream) {
  hipStream_t s = nullptr;
  int64_t nblock = 0;
  EPI_TRY(site_fetch_begin("epi_batch_linkage_blocks_fetch_dev", b, KIND_LINK, "epi_batch_linkage_blocks_dev", true, d_icols, 5, d_dcols, 1, stream, &s, &nblock));
  if (nblock == 0) return EPI_OK;
  LinkFinish f;
  link_finish_args(b, f);
  LinkBlockOut o;
  o.rname = d_icols[0]; o.strand = d_icols[1]; o.start = d_icols[2]; o.end = d_icols[3]; o.nsites = d_icols[4];
  o.mean_r2 = d_dcols[0];
  const unsigned nb = (unsigned)(((int64_t)f.N + SITE_WG - 1) / SITE_WG);
  hipLaunchKernelGGL(k_link_block_emit, dim3(nb), dim3(SITE_WG), 0, s, f, b->sites.link.blen.as<uint32_t>(), b->sites.link.bmean.as<double>(),
                     b->sites.link.bflag.as<uint32_t>(), b->sites.link.bout.as<uint32_t>(), o);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

}  // extern "C"
