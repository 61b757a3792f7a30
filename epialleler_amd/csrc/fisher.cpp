// rcpp_fep (src/rcpp_fep.cpp:10-36): two-sided Fisher exact p-values of 2x2 tables (a b / c d), host code.
// The reference calls HTSlib's kt_fisher_exact; this is written from the definition, and the arithmetic is in
// fisher_math.hpp (the definition is at its top), which the device kernels of cx_compare.hip share.
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <thread>
#include <vector>
#include "common.hpp"
#include "fisher_math.hpp"

using namespace epi;

extern "C" int epi_fisher_exact(const int32_t *a, const int32_t *b, const int32_t *c, const int32_t *d, int64_t n, double *p_out,
                                int nthreads) {
  if (n < 0 || (n > 0 && (!a || !b || !c || !d || !p_out))) return fail(EPI_ERR_ARG, "epi_fisher_exact: bad arguments");
  auto run = [&](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; i++) {
      // NA_integer_ (INT32_MIN) in any cell: NA (rcpp_fep.cpp:25-29); a negative count is no table either
      if (a[i] < 0 || b[i] < 0 || c[i] < 0 || d[i] < 0) { p_out[i] = NAN; continue; }
      p_out[i] = fisher::fisher_two_sided(a[i], b[i], c[i], d[i]);
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
