// The host side of the methylation-segment HMM (include/epihip.h, epi_cx_segment_dev, has the model): the quantisation of a
// model's parameters, the hard-EM re-estimate, and epi_segment_chain_host, the plain Viterbi loop over one chain.  All of it is
// on segment_math.hpp, which the kernels of segment.hip share; this unit is built without fast-math and without contraction
// (the Makefile pins it), so log, the one addition and the divisions are what the definitions say.
#include <math.h>
#include <stdint.h>
#include <vector>
#include "common.hpp"
#include "segment_math.hpp"

namespace epi {
namespace segment {

static int32_t quantise(double x) { return (int32_t)floor(log(x) * 65536.0 + 0.5); }

void quantise_tables(int K, const double *p, const double *trans, const double *init, int32_t *out) {
  for (int k = 0; k < K; k++) { out[k] = quantise(p[k]); out[K + k] = quantise(1.0 - p[k]); }
  for (int x = 0; x < K * K; x++) out[2 * K + x] = quantise(trans[x]);
  for (int k = 0; k < K; k++) out[2 * K + K * K + k] = quantise(init[k]);
}

void reestimate(int K, const int64_t *counts, double *p, double *trans, double *init) {
  const int64_t *M = counts, *U = counts + K, *N = counts + 2 * K, *S = counts + 2 * K + K * K;
  const double lo = 1.0 / 65536.0, hi = 1.0 - 1.0 / 65536.0;
  for (int k = 0; k < K; k++) {
    if (M[k] + U[k] == 0) continue;
    const double x = (double)(M[k] + 1) / (double)(M[k] + U[k] + 2);
    p[k] = x < lo ? lo : x > hi ? hi : x;
  }
  for (int j = 0; j < K; j++) {
    int64_t row = 0;
    for (int k = 0; k < K; k++) row += N[j * K + k];
    if (row == 0) continue;
    for (int k = 0; k < K; k++) trans[j * K + k] = (double)(N[j * K + k] + 1) / (double)(row + K);
  }
  int64_t starts = 0;
  for (int k = 0; k < K; k++) starts += S[k];
  for (int k = 0; k < K; k++) init[k] = (double)(S[k] + 1) / (double)(starts + K);
}

static bool in_range(double x, double lo, double hi) { return x >= lo && x <= hi; }   // (false for NaN)
static bool sums_to_one(const double *x, int K) {
  double s = 0.0;
  for (int k = 0; k < K; k++) s += x[k];
  return fabs(s - 1.0) <= 1e-9;
}

// the argument checks of a caller's model
int check_model(const char *who, int32_t K, const double *p, const double *trans, const double *init) {
  if (K < EPI_SEGMENT_MIN_STATES || K > EPI_SEGMENT_MAX_STATES)
    return fail(EPI_ERR_ARG, "%s: nstates = %d, from %d to %d", who, K, EPI_SEGMENT_MIN_STATES, EPI_SEGMENT_MAX_STATES);
  if (!p || !trans || !init) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  const double lo = 1.0 / 65536.0;
  for (int k = 0; k < K; k++)
    if (!in_range(p[k], lo, 1.0 - lo)) return fail(EPI_ERR_ARG, "%s: p[%d] = %g, from 2^-16 to 1 - 2^-16", who, k, p[k]);
  for (int x = 0; x < K * K; x++)
    if (!in_range(trans[x], lo, 1.0)) return fail(EPI_ERR_ARG, "%s: trans[%d][%d] = %g, from 2^-16 to 1", who, x / K, x % K, trans[x]);
  for (int k = 0; k < K; k++)
    if (!in_range(init[k], lo, 1.0)) return fail(EPI_ERR_ARG, "%s: init[%d] = %g, from 2^-16 to 1", who, k, init[k]);
  for (int j = 0; j < K; j++)
    if (!sums_to_one(trans + j * K, K)) return fail(EPI_ERR_ARG, "%s: row %d of trans does not sum to 1", who, j);
  if (!sums_to_one(init, K)) return fail(EPI_ERR_ARG, "%s: init does not sum to 1", who);
  return EPI_OK;
}

}  // namespace segment
}  // namespace epi

using namespace epi;

extern "C" {

int epi_segment_quantise(int32_t nstates, const double *p, const double *trans, const double *init, int32_t *tables_out) {
  EPI_TRY(segment::check_model("epi_segment_quantise", nstates, p, trans, init));
  if (!tables_out) return fail(EPI_ERR_ARG, "epi_segment_quantise: NULL argument");
  segment::quantise_tables(nstates, p, trans, init, tables_out);
  return EPI_OK;
}

int epi_segment_reestimate(int32_t nstates, const int64_t *counts, double *p, double *trans, double *init) {
  const char *who = "epi_segment_reestimate";
  if (nstates < EPI_SEGMENT_MIN_STATES || nstates > EPI_SEGMENT_MAX_STATES)
    return fail(EPI_ERR_ARG, "%s: nstates = %d, from %d to %d", who, nstates, EPI_SEGMENT_MIN_STATES, EPI_SEGMENT_MAX_STATES);
  if (!counts || !p || !trans || !init) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  for (int x = 0; x < segment::count_words(nstates); x++)
    if (counts[x] < 0 || counts[x] > (1LL << 42)) return fail(EPI_ERR_ARG, "%s: a count outside 0 .. 2^42", who);
  segment::reestimate(nstates, counts, p, trans, init);
  return EPI_OK;
}

}  // extern "C"

namespace {

template <int K>
void chain_loop(const segment::Tables &t, const int32_t *meth, const int32_t *unmeth, int64_t n, int32_t max_coverage, int32_t *state_out,
                int64_t *score_out) {
  std::vector<uint8_t> psi((size_t)n);
  segment::Vec<K> d, e;
  int32_t m, u;
  for (int64_t i = 0; i < n; i++) {
    segment::clip_counts(meth[i], unmeth[i], max_coverage, &m, &u);
    segment::emission<K>(t, m, u, e);
    if (i == 0) segment::first_step<K>(t, e, d);
    else psi[(size_t)i] = (uint8_t)segment::viterbi_step<K>(t, e, d);
  }
  uint32_t s = segment::best_state<K>(d, score_out);
  for (int64_t i = n - 1; i >= 0; i--) {
    state_out[i] = (int32_t)s;
    if (i > 0) s = segment::map_apply(psi[(size_t)i], s);
  }
}

}  // namespace

extern "C" int epi_segment_chain_host(int32_t nstates, const int32_t *tables, const int32_t *meth, const int32_t *unmeth, int64_t n,
                                      int32_t max_coverage, int32_t *state_out, int64_t *score_out) {
  const char *who = "epi_segment_chain_host";
  if (nstates < EPI_SEGMENT_MIN_STATES || nstates > EPI_SEGMENT_MAX_STATES)
    return fail(EPI_ERR_ARG, "%s: nstates = %d, from %d to %d", who, nstates, EPI_SEGMENT_MIN_STATES, EPI_SEGMENT_MAX_STATES);
  if (max_coverage < 1 || max_coverage > EPI_SEGMENT_MAX_COVERAGE)
    return fail(EPI_ERR_ARG, "%s: max_coverage = %d, from 1 to %d", who, max_coverage, EPI_SEGMENT_MAX_COVERAGE);
  if (n < 1 || n > EPI_SEGMENT_MAX_SITES) return fail(EPI_ERR_ARG, "%s: %lld sites, a chain holds 1 to 2^26", who, (long long)n);
  if (!tables || !meth || !unmeth || !state_out || !score_out) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  const int K = nstates;
  for (int x = 0; x < segment::table_words(K); x++)
    if (tables[x] > 0 || tables[x] < (x < 2 * K ? segment::kMinEmission : segment::kMinTable))
      return fail(EPI_ERR_ARG, "%s: table entry %d is %d: A and B lie in [%d, 0], T and I in [%d, 0]", who, x, tables[x], segment::kMinEmission,
                  segment::kMinTable);
  for (int64_t i = 0; i < n; i++)
    if (meth[i] < 0 || unmeth[i] < 0) return fail(EPI_ERR_ARG, "%s: a negative count", who);
  segment::Tables t = {};
  if (K == 2) { segment::tables_unpack<2>(tables, t); chain_loop<2>(t, meth, unmeth, n, max_coverage, state_out, score_out); }
  else if (K == 3) { segment::tables_unpack<3>(tables, t); chain_loop<3>(t, meth, unmeth, n, max_coverage, state_out, score_out); }
  else { segment::tables_unpack<4>(tables, t); chain_loop<4>(t, meth, unmeth, n, max_coverage, state_out, score_out); }
  return EPI_OK;
}
