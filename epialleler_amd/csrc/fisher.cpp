// rcpp_fep (src/rcpp_fep.cpp:10-36): two-sided Fisher exact p-values of 2x2 tables (a b / c d), host code.
// The reference calls HTSlib's kt_fisher_exact; this is written from the definition: with row sums n1 = a + b,
// n2 = c + d and first column m = a + c, the tables with the same margins are k = a' in [max(0, m - n2), min(m, n1)],
// P(k) = C(n1, k) C(n2, m - k) / C(n1 + n2, m), and the p-value is the sum of P(k) over the tables no more probable than
// the observed one, P(k) <= P(a) (1 + kRelTol) -- the relative tolerance makes tables whose probabilities are equal
// up to rounding count as "as extreme" (R's fisher.test and scipy use the same 1e-7).
// P(k) is evaluated in the saddle-point form of Loader ("Fast and accurate computation of binomial probabilities",
// 2000): no factorials, relative error ~1e-15 for cells of any size.  The hypergeometric distribution is unimodal, so
// the tables counted are two tails; each tail's inner end is found by bisection and the tail is summed outwards by the
// ratio recurrence until its terms no longer change the sum.
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <thread>
#include <vector>
#include "common.hpp"

namespace {

constexpr double kRelTol = 1e-7;
constexpr double kLn2Pi = 1.837877066409345483560659472811;   // log(2 pi)

// stirlerr(n) = log(n!) - log(sqrt(2 pi n) (n / e)^n)
double stirlerr(double n) {
  if (n <= 15.0) return lgamma(n + 1.0) - (n + 0.5) * log(n) + n - 0.5 * kLn2Pi;
  const double S0 = 1.0 / 12, S1 = 1.0 / 360, S2 = 1.0 / 1260, S3 = 1.0 / 1680, S4 = 1.0 / 1188;
  const double nn = n * n;
  if (n > 500) return (S0 - S1 / nn) / n;
  if (n > 80) return (S0 - (S1 - S2 / nn) / nn) / n;
  if (n > 35) return (S0 - (S1 - (S2 - S3 / nn) / nn) / nn) / n;
  return (S0 - (S1 - (S2 - (S3 - S4 / nn) / nn) / nn) / nn) / n;
}

// deviance term x log(x / np) + np - x, accurately also when x is close to np
double bd0(double x, double np) {
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
double dbinom_raw(double x, double n, double p, double q) {
  if (p == 0) return x == 0 ? 1.0 : 0.0;
  if (q == 0) return x == n ? 1.0 : 0.0;
  if (x == 0) {
    if (n == 0) return 1.0;
    return exp(p < 0.1 ? -bd0(n, n * q) - n * p : n * log(q));
  }
  if (x == n) return exp(q < 0.1 ? -bd0(n, n * p) - n * q : n * log(p));
  if (x < 0 || x > n) return 0.0;
  const double lc = stirlerr(n) - stirlerr(x) - stirlerr(n - x) - bd0(x, n * p) - bd0(n - x, n * q);
  const double lf = kLn2Pi + log(x) + log1p(-x / n);
  return exp(lc - 0.5 * lf);
}

struct Hyper {
  double n1, n2, m;             // rows sums, first column sum
  double p, q;
  double operator()(double k) const {            // P(k)
    return dbinom_raw(k, n1, p, q) * dbinom_raw(m - k, n2, p, q) / dbinom_raw(m, n1 + n2, p, q);
  }
  double up(double k) const { return (n1 - k) * (m - k) / ((k + 1) * (n2 - m + k + 1)); }     // P(k + 1) / P(k)
  double down(double k) const { return k * (n2 - m + k) / ((n1 - k + 1) * (m - k + 1)); }    // P(k - 1) / P(k)
};

double fisher_two_sided(int64_t a, int64_t b, int64_t c, int64_t d) {
  const int64_t n1 = a + b, n2 = c + d, m = a + c, n = n1 + n2;
  const int64_t lo = std::max<int64_t>(0, m - n2), hi = std::min(m, n1);
  if (lo == hi) return 1.0;
  Hyper f;
  f.n1 = (double)n1; f.n2 = (double)n2; f.m = (double)m;
  f.p = (double)m / (double)n; f.q = (double)(n - m) / (double)n;
  const double p0 = f((double)a);
  if (!(p0 > 0)) return 0.0;                     // the observed table's probability underflows: so does the sum
  const double thr = p0 * (1.0 + kRelTol);
  int64_t mode = (int64_t)floor(((double)m + 1) * ((double)n1 + 1) / ((double)n + 2));
  mode = std::min(std::max(mode, lo), hi);
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

}  // namespace

using namespace epi;

extern "C" int epi_fisher_exact(const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d, int64_t n, double *p_out,
                                int nthreads) {
  if (n < 0 || (n > 0 && (!a || !b || !c || !d || !p_out))) return fail(EPI_ERR_ARG, "epi_fisher_exact: bad arguments");
  auto run = [&](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; i++) {
      // NA_integer_ (INT32_MIN) in any cell: NA (rcpp_fep.cpp:25-29); a negative count is no table either
      if (a[i] < 0 || b[i] < 0 || c[i] < 0 || d[i] < 0) { p_out[i] = NAN; continue; }
      p_out[i] = fisher_two_sided(a[i], b[i], c[i], d[i]);
    }
  };
  int nt = nthreads > 1 ? std::min(nthreads, 64) : 1;
  if (n < 4096) nt = 1;
  std::vector<std::thread> th;
  for (int t = 1; t < nt; t++) th.emplace_back(run, n * t / nt, n * (t + 1) / nt);
  run(0, n / nt);
  for (auto &t : th) t.join();
  return EPI_OK;
}
