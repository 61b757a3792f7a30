// Tail probabilities of the chi-square, Student and F(1, df) distributions, shared by the host entry point (dist.cpp,
// epi_dist_tail) and the device kernels (cx_groups.hip): one copy, the same operations in the same order on either side,
// as with fisher_math.hpp, whose stirlerr and bd0 this builds on.
//   chisq_upper(x, df) = Q(df / 2, x / 2), the regularised upper incomplete gamma function.  With a = df / 2, z = x / 2 and
//                        D = z^a e^-z / Gamma(a + 1) in Loader's form exp(-stirlerr(a) - bd0(a, z)) / sqrt(2 pi a) (no
//                        a log z - z - lgamma(a + 1), which cancels 4 digits at a = 5000):
//                        z < a + 1:  1 - D (1 + z / (a + 1) + z^2 / ((a + 1)(a + 2)) + ...)
//                        otherwise:  D a / (z + 1 - a - 1 (1 - a) / (z + 3 - a - 2 (2 - a) / (z + 5 - a - ...))), modified Lentz;
//                        df == 1:    erfc(sqrt(z)).
//   beta_tail(s, df)   = I_x(df / 2, 1 / 2) with x = df / (df + s), the regularised incomplete beta function: the two-sided
//                        tail of Student's t for s = t^2 and the upper tail of F(1, df) for s = F.  With a = df / 2, b = 1 / 2,
//                        y = s / (df + s) (formed directly: 1 - x would cancel) and B = x^a y^b / Beta(a, b):
//                        x < (a + 1) / (a + b + 2):  B cf(a, b, x) / a
//                        otherwise:                  1 - B cf(b, a, y) / b        (the symmetric swap)
//                        cf is the continued fraction of the incomplete beta function (Abramowitz & Stegun 26.5.8) by the
//                        modified Lentz method.  log x and log y are log1p(-y) and log1p(-x) where the argument is above 1 / 2,
//                        and log(Gamma(a + 1/2) / Gamma(a)) is formed from stirlerr differences: the difference of two lgamma
//                        values of size 37 000 is good to 4e-12 only.
// Domain: 0 < df <= kMaxDf = 1e4 and finite; x, s >= 0.  0 gives 1, +inf gives 0; NaN, a negative value or a df outside the
// range gives NaN.
// Every loop has a fixed bound, derived next to it; a tail that has not converged at its bound is NaN, never a longer loop.
// Against mpmath at 50 digits (tests/test_dist_host.py: the grid x, t in {0, 1e-8, 0.1, 1, 2, 3.84, 5, 10, 37, 100, 1e3,
// 1400} x df in {1, 1.5, 2, 3.7, 10, 30, 63, 100, 1e3, 1e4} and 600 seeded random points, where the exact value is at least
// 1e-300) the host's largest relative error is 6.4e-13: beta_tail(4, 1e4), just below the swap, where the denominators of
// the direct fraction cancel (the swapped form is good to 2.5e-14 there, but loses 1 / p digits further out); 1e-13 or less
// from df = 1e3 down.  chisq_upper's is 1.1e-13, at p = 4e-249: a p-value is the exponential of a sum, so its relative error
// is about 1e-16 times the size of the exponent.
// Every translation unit that includes this is compiled with -fno-fast-math -ffp-contract=off.
#pragma once
#include "../../include/epihip.h"
#include "fisher_math.hpp"

namespace epi {
namespace dist {

constexpr double kMaxDf = 1e4;
constexpr double kLnPi = 1.144729885849400174143427351353;   // log(pi)
constexpr double kTiny = 1e-300;                             // Lentz: what a vanishing denominator is replaced by
constexpr double kCfEps = 4.440892098500626e-16;             // 2^-51: a factor this close to 1 ends a continued fraction

// Iteration bounds (a = df / 2 <= 5000 on the domain).
// Series: below the switch z < a + 1 the n-th term is at most prod_{k=1..n} (a + 1) / (a + k), whose logarithm is
//   -sum_{j<n} log(1 + j / (a + 1)) <= -(n^2 / (2 (a + 1)) - n^3 / (6 (a + 1)^2)); at a = 5000 and n = 700 that is -46.7,
//   below log(2^-53) = -36.7, and smaller a converge sooner: 1000 terms always suffice.
// Continued fractions: both converge in O(sqrt(a)) steps next to their switch and faster away from it.  Counted over the
//   domain (a sweep of 9.6e5 points, densest next to the switches; scratch/dist_iterations.py): at most 152 steps for the
//   gamma fraction and 78 for the beta fraction, both at a = 5000 next to the switch (the series: 578 terms); the bounds
//   are more than twice that.
constexpr int kSeriesMax = 1000;
constexpr int kGammaCfMax = 400;
constexpr int kBetaCfMax = 200;
constexpr int kBetaShift = 16;                              // ln_beta_half: a <= 15 becomes a + 16, where stirlerr is a series

#ifdef EPI_DIST_COUNT_STEPS
static int g_steps[3];                                       // (scratch/dist_iterations.py: the most steps each loop took)
#define EPI_DIST_STEPS(which, n) do { if ((n) > g_steps[which]) g_steps[which] = (n); } while (0)
#else
#define EPI_DIST_STEPS(which, n) do { } while (0)
#endif

// z^a e^-z / Gamma(a + 1), a > 0, z > 0
EPI_FISHER_HD static double pois_term(double a, double z) {
  return exp(-fisher::stirlerr(a) - fisher::bd0(a, z)) / sqrt(2.0 * 3.141592653589793238462643383279 * a);
}

EPI_FISHER_HD static double chisq_upper(double x, double df) {
  if (!(df > 0.0 && df <= kMaxDf) || !(x >= 0.0)) return __builtin_nan("");
  if (x == 0.0) return 1.0;
  if (__builtin_isinf(x)) return 0.0;
  const double z = 0.5 * x, a = 0.5 * df;
  if (df == 1.0) return erfc(sqrt(z));
  const double D = pois_term(a, z);
  if (z < a + 1.0) {
    double sum = 1.0, t = 1.0;
    for (int n = 1; n <= kSeriesMax; n++) {
      t *= z / (a + n);
      const double s1 = sum + t;
      if (s1 == sum) {
        EPI_DIST_STEPS(0, n);
        const double q = 1.0 - D * sum;
        return q < 0.0 ? 0.0 : q;
      }
      sum = s1;
    }
    return __builtin_nan("");
  }
  double b = z + 1.0 - a, c = 1.0 / kTiny, d = 1.0 / b, h = d;   // (b >= 2 here)
  for (int i = 1; i <= kGammaCfMax; i++) {
    const double an = -(double)i * ((double)i - a);
    b += 2.0;
    d = an * d + b;
    if (fabs(d) < kTiny) d = kTiny;
    c = b + an / c;
    if (fabs(c) < kTiny) c = kTiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) <= kCfEps) {
      EPI_DIST_STEPS(1, i);
      const double q = D * a * h;
      return q > 1.0 ? 1.0 : q;
    }
  }
  return __builtin_nan("");
}

// the continued fraction of I_x(a, b)
EPI_FISHER_HD static double beta_cf(double a, double b, double x) {
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (fabs(d) < kTiny) d = kTiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= kBetaCfMax; m++) {
    const double m2 = 2.0 * m;
    double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < kTiny) d = kTiny;
    c = 1.0 + aa / c;
    if (fabs(c) < kTiny) c = kTiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < kTiny) d = kTiny;
    c = 1.0 + aa / c;
    if (fabs(c) < kTiny) c = kTiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) <= kCfEps) {
      EPI_DIST_STEPS(2, m);
      return h;
    }
  }
  return __builtin_nan("");
}

// log(Gamma(a + 1/2) / (Gamma(a) Gamma(1/2))) from stirlerr differences.  a <= 15 is first raised by kBetaShift:
// Gamma(a + 1/2) / Gamma(a) = Gamma(a + n + 1/2) / Gamma(a + n) * prod_{k<n} (a + k) / (a + k + 1/2) -- no lgamma (two
// calls of the device's cost the kernels 16 bytes of scratch memory per lane): u and v below are above 15, stirlerr's series.
EPI_FISHER_HD static double ln_beta_half(double a) {
  double shift = 0.0;
  if (a <= 15.0) {
    double r = 1.0;
    for (int k = 0; k < kBetaShift; k++) r *= (a + k) / (a + k + 0.5);
    shift = log(r);
    a += kBetaShift;
  }
  const double u = a - 0.5, v = a - 1.0;                     // Gamma(a + 1/2) = u!, Gamma(a) = v!
  return shift + (fisher::stirlerr_series(u) - fisher::stirlerr_series(v) + 0.5 * log(u / v) + u * log1p(0.5 / v) + 0.5 * log(v) - 0.5 - 0.5 * kLnPi);
}

EPI_FISHER_HD static double beta_tail(double s, double df) {
  if (!(df > 0.0 && df <= kMaxDf) || !(s >= 0.0)) return __builtin_nan("");
  if (s == 0.0) return 1.0;
  if (__builtin_isinf(s)) return 0.0;
  const double a = 0.5 * df, b = 0.5, t = df + s;
  double x = df / t, y = s / t;
  if (__builtin_isinf(t)) { x = df / s; y = 1.0; }
  const double lx = y < 0.5 ? log1p(-y) : log(x), ly = x < 0.5 ? log1p(-x) : log(y);
  const double B = exp(ln_beta_half(a) + a * lx + b * ly);
  if (x < (a + 1.0) / (a + b + 2.0)) {
    const double p = B * beta_cf(a, b, x) / a;
    return p > 1.0 ? 1.0 : p;
  }
  const double p = 1.0 - B * beta_cf(b, a, y) / b;
  return p < 0.0 ? 0.0 : p;
}

// epi_dist_tail's value for one element (include/epihip.h): the chi-square tail of x, the two-sided Student tail of the
// statistic t = x (either sign), the F(1, df) tail of x
EPI_FISHER_HD static double tail_of(int32_t kind, double x, double df) {
  if (kind == EPI_DIST_CHISQ) return chisq_upper(x, df);
  if (kind == EPI_DIST_T2) return beta_tail(x * x, df);
  return beta_tail(x, df);
}

}  // namespace dist
}  // namespace epi
