// epi_smooth_window: the smoother's fit of one window, host code.  The arithmetic is in smooth_math.hpp (the definitions are
// at its top), which the device kernel of smooth.hip shares.
#include <stdint.h>
#include "common.hpp"
#include "smooth_math.hpp"

using namespace epi;

extern "C" int epi_smooth_window(const int32_t *pos, const int32_t *meth, const int32_t *unmeth, int64_t n, int64_t i, int32_t halfwidth,
                                 int32_t degree, double *smoothed, int32_t *degree_used, double *weight) {
  const char *who = "epi_smooth_window";
  if (!pos || !meth || !unmeth || !smoothed || !degree_used || !weight) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  if (n < 1 || i < 0 || i >= n) return fail(EPI_ERR_ARG, "%s: site %lld of %lld", who, (long long)i, (long long)n);
  if (halfwidth < 1) return fail(EPI_ERR_ARG, "%s: halfwidth = %d, at least 1", who, halfwidth);
  if (degree < 0 || degree > EPI_SMOOTH_MAX_DEGREE) return fail(EPI_ERR_ARG, "%s: degree = %d, from 0 to %d", who, degree, EPI_SMOOTH_MAX_DEGREE);
  smooth::Sums s;
  smooth::sums_zero(s);
  const double H = (double)halfwidth;
  for (int64_t j = 0; j < n; j++) {                           // ascending j
    if (meth[j] < 0 || unmeth[j] < 0) return fail(EPI_ERR_ARG, "%s: a negative count", who);
    const int64_t d = (int64_t)pos[j] - (int64_t)pos[i];
    if (d <= -(int64_t)halfwidth || d >= (int64_t)halfwidth) continue;
    smooth::sums_add(s, d, H, meth[j], (uint32_t)meth[j] + (uint32_t)unmeth[j]);
  }
  int used = 0;
  *smoothed = smooth::solve(s, degree, &used);
  *degree_used = used;
  *weight = s.S0;
  return EPI_OK;
}
