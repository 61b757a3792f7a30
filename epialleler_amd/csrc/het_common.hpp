// What the heterogeneity report (heterogeneity.hip) and the heterogeneity comparison (het_compare.hip) share on top of the
// site table (site_table.hpp): the windows of k sites over it, the metrics of a window's histogram, the counting kernel's
// launch (the comparison counts two batches with it on the sites both have) and the checks of the entry points.
#pragma once
#include "site_table.hpp"

namespace epi {

struct HetFinish : SiteView {           // the site table with the windows of a heterogeneity report or a comparison
  uint32_t N;
  int32_t k;
  uint32_t min_reads;
  int64_t max_span;
};

// the window that starts at CX row i: its counters, or null when fewer than k sites follow on its (rname, strand)
__device__ __forceinline__ const uint32_t *het_window(const HetFinish &f, uint32_t i, int32_t *end) {
  const int32_t st = f.strand[i];
  const uint32_t n1 = *f.n1;
  const uint32_t g = site_ordinal(st, i, f.rank[i], n1), seg_end = st == 1 ? n1 : f.N;
  const uint32_t last = g + (uint32_t)f.k - 1u;
  if (last >= seg_end) return nullptr;
  const unsigned long long kl = f.key[last];
  if ((uint32_t)(kl >> 32) != (uint32_t)f.rname[i]) return nullptr;
  *end = table_key_pos(kl);
  return f.counts + ((size_t)g << f.k);
}

// What one histogram c[2^k] says of its sample.  The bin sums run over the bins in ascending order inside one thread; hist,
// when given, receives the histogram as a row of int32.
struct HetMetrics {
  uint64_t n;
  int32_t npatterns;
  double beta, epipoly, entropy, pdr;
};
__device__ __forceinline__ HetMetrics het_metrics(const uint32_t *c, int k, int32_t *hist) {
  const int nb = 1 << k;
  uint64_t n = 0, nmeth = 0;
  int32_t npat = 0;
  for (int b = 0; b < nb; b++) { const uint32_t v = c[b]; n += v; nmeth += (uint64_t)v * (uint32_t)__popc(b); npat += v ? 1 : 0; }
  const double dn = (double)n;
  double sq = 0.0, ent = 0.0;
  for (int b = 0; b < nb; b++) {                              // ascending bins
    const uint32_t v = c[b];
    if (hist) hist[b] = (int32_t)v;
    if (!v) continue;
    const double pb = (double)v / dn;
    sq += pb * pb;
    ent += pb * log2(pb);
  }
  HetMetrics m;
  m.n = n; m.npatterns = npat;
  m.beta = (double)nmeth / (dn * (double)k);
  m.epipoly = 1.0 - sq;
  m.entropy = -ent / (double)k;
  m.pdr = 1.0 - (double)((uint64_t)c[0] + c[nb - 1]) / dn;
  return m;
}

constexpr int kHetMinK = 2, kHetMaxK = 6;
// bytes of counters (nsites * 2^k * 4) of a heterogeneity report or of one side of a comparison, or -1 when a report
// refuses them: above 4 GiB, or sites beyond 32-bit ordinals
int64_t het_counter_bytes(int64_t nsites, int k);

// the site table of b with window size and thresholds of the last report on it
void het_finish_args(const epi_batch *b, HetFinish &f);
// k and max_window_span as a report and a comparison take them (`who`: the entry point, for the message)
int het_check_window(const char *who, int k, int32_t max_window_span);
// k_het_count<16> or <64> (heterogeneity.hip): the rows of `a` add to counts [a.N << k], which the caller has zeroed;
// nb_rows and wide are site_count_blocks' of the batch the rows are of
int het_count_launch(const SiteRows &a, int k, uint32_t *counts, int64_t nb_rows, bool wide, hipStream_t s);

}  // namespace epi
