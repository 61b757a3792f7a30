// The arithmetic of the two-sided Fisher exact test of a 2x2 table (a b / c d), shared by the host entry point
// (fisher.cpp, epi_fisher_exact) and the device kernels (cx_compare.hip): one copy, the same operations in the same order
// on either side.  With row sums n1 = a + b, n2 = c + d and first column m = a + c, the tables with the same margins are
// k = a' in [max(0, m - n2), min(m, n1)], P(k) = C(n1, k) C(n2, m - k) / C(n1 + n2, m), and the p-value is the sum of P(k)
// over the tables no more probable than the observed one, P(k) <= P(a) (1 + kRelTol) -- the relative tolerance makes tables
// whose probabilities are equal up to rounding count as "as extreme" (R's fisher.test and scipy use the same 1e-7).
// P(k) is evaluated in the saddle-point form of Loader ("Fast and accurate computation of binomial probabilities",
// 2000): no factorials.  P is the exponential of a sum of terms each good to an ulp or so, so its relative error is
// about 1e-16 times the size of the exponent: against a 60-digit sum over tables with cells up to 2^31 - 1
// (tests/test_cx_compare_host.py::test_fisher_host_against_exact_arithmetic) p is off by at most 1.0e-13, at
// p = 9e-122, and by a few 1e-15 where p is of ordinary size.  The hypergeometric distribution is unimodal, so
// the tables counted are two tails; each tail's inner end is found by bisection and the tail is summed outwards by the
// ratio recurrence until its terms no longer change the sum.
// Every translation unit that includes this is compiled with -fno-fast-math -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define EPI_FISHER_HD __host__ __device__
#else
#define EPI_FISHER_HD
#endif

namespace epi {
namespace fisher {

constexpr double kRelTol = 1e-7;
constexpr double kLn2Pi = 1.837877066409345483560659472811;   // log(2 pi)

// stirlerr(n) = log(n!) - log(sqrt(2 pi n) (n / e)^n): its series, n > 15 (dist_math.hpp calls this half alone)
EPI_FISHER_HD static double stirlerr_series(double n) {
  const double S0 = 1.0 / 12, S1 = 1.0 / 360, S2 = 1.0 / 1260, S3 = 1.0 / 1680, S4 = 1.0 / 1188;
  const double nn = n * n;
  if (n > 500) return (S0 - S1 / nn) / n;
  if (n > 80) return (S0 - (S1 - S2 / nn) / nn) / n;
  if (n > 35) return (S0 - (S1 - (S2 - S3 / nn) / nn) / nn) / n;
  return (S0 - (S1 - (S2 - (S3 - S4 / nn) / nn) / nn) / nn) / n;
}

EPI_FISHER_HD static double stirlerr(double n) {
  if (n <= 15.0) return lgamma(n + 1.0) - (n + 0.5) * log(n) + n - 0.5 * kLn2Pi;
  return stirlerr_series(n);
}

// deviance term x log(x / np) + np - x, accurately also when x is close to np
EPI_FISHER_HD static double bd0(double x, double np) {
  if (fabs(x - np) < 0.1 * (x + np)) {
    double v = (x - np) / (x + np);
    double s = (x - np) * v, ej = 2 * x * v;
    v *= v;
    for (int j = 1; j < 1000; j++) {
      ej *= v;
      const double s1 = s + ej / (2 * j + 1);
      if (s1 == s) return s1;
      s = s1;
    }
    return s;
  }
  return x * log(x / np) + np - x;
}

// binomial probability of x in n trials, success p (q = 1 - p)
EPI_FISHER_HD static double dbinom_raw(double x, double n, double p, double q) {
  if (p == 0) return x == 0 ? 1.0 : 0.0;
  if (q == 0) return x == n ? 1.0 : 0.0;
  if (x == 0) {
    if (n == 0) return 1.0;
    return exp(p < 0.1 ? -bd0(n, n * q) - n * p : n * log(q));
  }
  if (x == n) return exp(q < 0.1 ? -bd0(n, n * p) - n * q : n * log(p));
  if (x < 0 || x > n) return 0.0;
  const double lc = stirlerr(n) - stirlerr(x) - stirlerr(n - x) - bd0(x, n * p) - bd0(n - x, n * q);
  const double lf = kLn2Pi + log(x) + log((n - x) / n);    // (n - x is exact; 1 - x / n loses its digits when x is close to n)
  return exp(lc - 0.5 * lf);
}

struct Hyper {
  double n1, n2, m;             // rows sums, first column sum
  double p, q;
  EPI_FISHER_HD double operator()(double k) const {            // P(k)
    return dbinom_raw(k, n1, p, q) * dbinom_raw(m - k, n2, p, q) / dbinom_raw(m, n1 + n2, p, q);
  }
  EPI_FISHER_HD double up(double k) const { return (n1 - k) * (m - k) / ((k + 1) * (n2 - m + k + 1)); }     // P(k + 1) / P(k)
  EPI_FISHER_HD double down(double k) const { return k * (n2 - m + k) / ((n1 - k + 1) * (m - k + 1)); }    // P(k - 1) / P(k)
};

// non-negative cells (the callers turn a negative one into NaN); dist.cpp includes this header for stirlerr and bd0 alone
[[maybe_unused]] EPI_FISHER_HD static double fisher_two_sided(int64_t a, int64_t b, int64_t c, int64_t d) {
  const int64_t n1 = a + b, n2 = c + d, m = a + c, n = n1 + n2;
  const int64_t lo = m - n2 > 0 ? m - n2 : 0, hi = m < n1 ? m : n1;
  if (lo == hi) return 1.0;
  Hyper f;
  f.n1 = (double)n1; f.n2 = (double)n2; f.m = (double)m;
  f.p = (double)m / (double)n; f.q = (double)(n - m) / (double)n;
  const double p0 = f((double)a);
  if (!(p0 > 0)) return 0.0;                     // the observed table's probability underflows: so does the sum
  const double thr = p0 * (1.0 + kRelTol);
  int64_t mode = (int64_t)floor(((double)m + 1) * ((double)n1 + 1) / ((double)n + 2));
  mode = mode > lo ? mode : lo;
  mode = mode < hi ? mode : hi;
  if (f((double)mode) <= thr) return 1.0;        // every table is as extreme
  // left tail [lo, kl): P is non-decreasing on [lo, mode]; kl = first k there with P(k) > thr
  int64_t x0 = lo, x1 = mode;
  while (x0 < x1) { const int64_t k = x0 + (x1 - x0) / 2; if (f((double)k) > thr) x1 = k; else x0 = k + 1; }
  const int64_t kl = x0;
  // right tail (kr, hi]: P is non-increasing on [mode, hi]; kr = last k there with P(k) > thr
  x0 = mode; x1 = hi;
  while (x0 < x1) { const int64_t k = x0 + (x1 - x0 + 1) / 2; if (f((double)k) > thr) x0 = k; else x1 = k - 1; }
  const int64_t kr = x0;
  double sum = 0.0;
  if (kl > lo) {                                 // outwards from kl - 1 down to lo
    double t = f((double)(kl - 1));
    double s = 0.0;
    for (int64_t k = kl - 1; k >= lo; k--) {
      const double s1 = s + t;
      if (s1 == s) break;                        // (log-concave: the terms only shrink from here on)
      s = s1;
      t *= f.down((double)k);
    }
    sum += s;
  }
  if (kr < hi) {
    double t = f((double)(kr + 1));
    double s = 0.0;
    for (int64_t k = kr + 1; k <= hi; k++) {
      const double s1 = s + t;
      if (s1 == s) break;
      s = s1;
      t *= f.up((double)k);
    }
    sum += s;
  }
  return sum > 1.0 ? 1.0 : sum;
}

}  // namespace fisher
}  // namespace epi
