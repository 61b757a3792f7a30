// The arithmetic of the local-regression smoother of a cytosine report (include/epihip.h, epi_cx_smooth_dev, has the
// definitions), shared by the host entry point (smooth_host.cpp, epi_smooth_window) and the device kernel (smooth.hip): one copy,
// the same operations in the same order on either side, as with fisher_math.hpp and dist_math.hpp.
//   Window   site i with half-width H: the sites j with |pos_j - pos_i| < H, visited in ascending j by ONE thread.  Per site
//            d = pos_j - pos_i (an integer, exact in a double), u = d / H, a = |u|, tricube weight t = (1 - a^3)^3, and the
//            eight sums S0 .. S4 = sum of w u^k with w = t (meth_j + unmeth_j), T0 .. T2 = sum of v u^k with v = t meth_j:
//            the weighted normal equations of a polynomial in u fitted to the sites' betas with weights t * coverage.
//   Solve    the intercept (the fit at u = 0) by an LDL^T factorisation of the moment matrix [S0 S1 S2; S1 S2 S3; S2 S3 S4].
//            A pivot is accepted when it is above kPivot times its own diagonal element (d1 against S2, d2 against S4): the
//            pivot is what is left of that element once the lower orders are projected out, so the test is relative and
//            free of the scale of the coverage.  A refused pivot lowers the degree.  kPivot = 1e-4 is conservative: one-sided
//            windows at a cluster's end extrapolate from nearly collinear points, where a small pivot amplifies rounding.
//            Against exact rational arithmetic the worst absolute error of the intercept over tests/test_smooth_host.py's
//            seeded series is 1.8e-12 (5.2e-12 with 1e-6, 1.0e-11 with 1e-8 in place of the constant).
// Every product and every sum below is one correctly rounded IEEE operation in the order written: every translation unit
// that includes this is compiled with -fno-fast-math -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define EPI_SMOOTH_HD __host__ __device__
#else
#define EPI_SMOOTH_HD
#endif

namespace epi {
namespace smooth {

constexpr double kPivot = 1e-4;

struct Sums { double S0, S1, S2, S3, S4, T0, T1, T2; };      // eight independent chains

EPI_SMOOTH_HD static inline void sums_zero(Sums &s) { s.S0 = s.S1 = s.S2 = s.S3 = s.S4 = s.T0 = s.T1 = s.T2 = 0.0; }

// one window site: d = pos_j - pos_i, |d| < H; cov = meth + unmeth
EPI_SMOOTH_HD static inline void sums_add(Sums &s, int64_t d, double H, int32_t meth, uint32_t cov) {
  const double u = (double)d / H;
  const double a = fabs(u);
  const double c = 1.0 - (a * a) * a;
  const double t = (c * c) * c;
  const double u2 = u * u;
  const double w = t * (double)cov;
  const double v = t * (double)meth;
  const double wu2 = w * u2, vu2 = v * u2;
  s.S0 += w; s.S1 += w * u; s.S2 += wu2; s.S3 += wu2 * u; s.S4 += wu2 * u2;
  s.T0 += v; s.T1 += v * u; s.T2 += vu2;
}

// the fit at u = 0, clamped to [0, 1]; *degree_used: -1 (no coverage in the window, NaN), 0, 1 or 2
EPI_SMOOTH_HD static inline double solve(const Sums &s, int degree, int *degree_used) {
  if (!(s.S0 > 0.0)) { *degree_used = -1; return __builtin_nan(""); }
  const double d0 = s.S0;
  const double l10 = s.S1 / d0;
  const double d1 = s.S2 - l10 * s.S1;
  int used = 0;
  double l20 = 0.0, l21 = 0.0, d2 = 0.0;
  if (degree >= 1 && d1 > kPivot * s.S2) {
    used = 1;
    if (degree == 2) {
      l20 = s.S2 / d0;
      l21 = (s.S3 - l20 * s.S1) / d1;
      d2 = (s.S4 - l20 * s.S2) - l21 * (l21 * d1);
      if (d2 > kPivot * s.S4) used = 2;
    }
  }
  *degree_used = used;
  double a0;
  if (used == 0) {
    a0 = s.T0 / d0;
  } else {
    const double z1 = s.T1 - l10 * s.T0;
    if (used == 1) {
      const double a1 = z1 / d1;
      a0 = s.T0 / d0 - l10 * a1;
    } else {
      const double z2 = (s.T2 - l20 * s.T0) - l21 * z1;
      const double a2 = z2 / d2;
      const double a1 = z1 / d1 - l21 * a2;
      a0 = (s.T0 / d0 - l10 * a1) - l20 * a2;
    }
  }
  return fmin(1.0, fmax(0.0, a0));
}

}  // namespace smooth
}  // namespace epi
