// The most steps each loop of csrc/dist_math.hpp takes over its domain (scratch/dist_iterations.py builds and runs this).
#define EPI_DIST_COUNT_STEPS
#include <stdio.h>
#include "../epialleler_amd/csrc/dist_math.hpp"
using namespace epi::dist;

int main() {
  long npoints = 0, nan = 0;
  // a = df / 2 on a geometric ladder up to 5000; the argument on a ladder and, densely, around the switches
  for (double df = 0.01; df <= kMaxDf * 1.0000001; df *= 1.02) {
    const double d = df > kMaxDf ? kMaxDf : df, a = 0.5 * d;
    for (double x = 1e-6; x < 1e6; x *= 1.1) { npoints += 2; nan += chisq_upper(x, d) != chisq_upper(x, d); nan += beta_tail(x, d) != beta_tail(x, d); }
    for (int k = -200; k <= 200; k++) {
      const double z = (a + 1.0) * (1.0 + k * 1e-4);           // the gamma switch z = a + 1
      const double xs = (a + 1.0) / (a + 2.5) * (1.0 + k * 1e-5);   // the beta switch x = (a + 1) / (a + b + 2): s = df (1 - x) / x
      npoints += 2;
      nan += chisq_upper(2.0 * z, d) != chisq_upper(2.0 * z, d);
      if (xs < 1.0) nan += beta_tail(d * (1.0 - xs) / xs, d) != beta_tail(d * (1.0 - xs) / xs, d);
    }
  }
  printf("points %ld  not converged %ld  most steps: series %d  gamma fraction %d  beta fraction %d\n", npoints, nan, g_steps[0], g_steps[1], g_steps[2]);
  return 0;
}
