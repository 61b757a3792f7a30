// epi_dist_tail: tail probabilities of the chi-square, Student and F(1, df) distributions, host code.  The arithmetic is in
// dist_math.hpp (the definitions are at its top), which the device kernels of cx_groups.hip share.
#include <stdint.h>
#include "common.hpp"
#include "dist_math.hpp"

using namespace epi;

extern "C" int epi_dist_tail(int32_t kind, const double *x, const double *df, int64_t n, double *p_out) {
  if (kind < EPI_DIST_CHISQ || kind > EPI_DIST_F1) return fail(EPI_ERR_ARG, "epi_dist_tail: kind = %d, one of EPI_DIST_CHISQ, EPI_DIST_T2, EPI_DIST_F1", kind);
  if (n < 0 || (n > 0 && (!x || !df || !p_out))) return fail(EPI_ERR_ARG, "epi_dist_tail: bad arguments");
  for (int64_t i = 0; i < n; i++) p_out[i] = dist::tail_of(kind, x[i], df[i]);
  return EPI_OK;
}
