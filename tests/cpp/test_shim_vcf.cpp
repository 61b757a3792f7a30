// Driver for the generateVcfReport half of the shim core (epialleler_amd/r/epihip_shim_core.hpp), run by
// tests/test_shim_vcf.py:  test_shim_vcf cpu   -- fep_into (host code: rcpp_fep's conversions and NA rule)
//                          test_shim_vcf gpu   -- base_freqs_into on hand-made templates, every count checked
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "epihip_shim_core.hpp"

using namespace epihip_shim;

#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static int run_cpu() {
  // int columns (R integers) and double columns (the report's numeric columns, NA_real_ = NaN)
  const int32_t a[] = {3, 0, INT32_MIN, 5}, b[] = {1, 0, 1, 0}, c[] = {1, 0, 2, 0}, d[] = {3, 0, 3, 5};
  double p[4];
  fep_into(a, b, c, d, 4, p);
  EXPECT(fabs(p[0] - 0.4857142857142857) < 1e-12 && p[1] == 1.0 && isnan(p[2]) && fabs(p[3] - 2.0 / 252) < 1e-15);
  const double da[] = {3, NAN}, db[] = {1, 1}, dc[] = {1, 1}, dd[] = {3, 1};
  double q[2];
  fep_into(da, db, dc, dd, 2, q);
  EXPECT(q[0] == p[0] && isnan(q[1]));
  printf("shim vcf cpu ok\n");
  return 0;
}

static uint8_t byte(char base) {               // (nt16 << 4) | a context code; only the base matters here
  const int nt = base == 'A' ? 1 : base == 'C' ? 2 : base == 'G' ? 4 : base == 'T' ? 8 : 15;
  return (uint8_t)((nt << 4) | 12);
}

static int run_gpu() {
  // three templates on rname 1 (the third on the '-' strand, failing), one on rname 2; rows sorted by (rname, start)
  const std::vector<std::string> seq = {"ACGTN", "GGTTA", "CCCCC", "TTTT"};
  std::vector<std::string> xm;
  for (const std::string &t : seq) { std::string s; for (char ch : t) s += (char)byte(ch); xm.push_back(s); }
  const int32_t templid[] = {0, 1, 2, 3}, rname[] = {1, 1, 1, 2}, strand[] = {1, 1, 2, 1}, start[] = {10, 12, 13, 10};
  const int32_t pass[] = {1, INT32_MIN, 0, 1};
  Soa s;
  gather_rows(xm, templid, 4, s, []() {});
  // sites: (1,10) (1,12) (1,12) NA (1,14) (2,13) (3,1)
  const int32_t vchr[] = {1, 1, 1, INT32_MIN, 1, 2, 3}, vpos[] = {10, 12, 12, 12, 14, 13, 1};
  const int64_t m = 7;
  std::vector<double> out((size_t)m * 20, -1.0);
  base_freqs_into(s, rname, strand, start, 4, pass, vchr, vpos, m, out.data());
  auto at = [&](int i, int col) { return out[(size_t)col * m + i]; };
  double want[7][20];
  memset(want, 0, sizeof(want));
  // col = base + (strand - 1) * 5 + pass * 10; A C G T N = 0 1 2 3 4
  want[0][10 + 0] = 1;                         // read 0 at 10: A, '+', pass
  want[1][10 + 2] = 1; want[2][10 + 2] = 1;    // read 0 at 12: G (both multi-ALT rows)
  want[1][10 + 2] += 1; want[2][10 + 2] += 1;  // read 1 at 12: G, pass NA = TRUE
  want[4][10 + 4] = 1;                         // read 0 at 14: N
  want[4][10 + 3] = 1;                         // read 1 at 14: T
  want[4][5 + 1] = 1;                          // read 2 at 14: C, '-', no pass
  want[5][10 + 3] = 1;                         // read 3 at 13 on rname 2: T
  for (int i = 0; i < m; i++)
    for (int c = 0; c < 20; c++)
      if (at(i, c) != want[i][c]) { fprintf(stderr, "site %d col %d: %g != %g\n", i, c, at(i, c), want[i][c]); return 1; }
  const int32_t uchr[] = {1, 1}, upos[] = {14, 10};
  bool thrown = false;
  try { base_freqs_into(s, rname, strand, start, 4, pass, uchr, upos, 2, out.data()); } catch (const std::exception &) { thrown = true; }
  EXPECT(thrown);
  printf("shim vcf gpu ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  if (!strcmp(argv[1], "cpu")) return run_cpu();
  if (!strcmp(argv[1], "gpu")) return run_gpu();
  return 2;
}
