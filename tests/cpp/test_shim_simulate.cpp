// Driver for simulateBam's half of the shim core (epialleler_amd/r/epihip_shim_core.hpp: sim_columns, simulate_bam), run
// by tests/test_shim_simulate.py:  test_shim_simulate cpu       -- the columns R's data.frames become (host code)
//                                  test_shim_simulate gpu OUT   -- simulate_bam with the table of shim_case()
#include <stdio.h>
#include <string.h>
#include <stdexcept>
#include <string>
#include <vector>
#include "epihip_shim_core.hpp"

using namespace epihip_shim;

#define EXPECT(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// what .simulateBam hands rcpp_simulate_bam for the call in tests/test_shim_simulate.py (every column recycled to 3)
static void shim_case(std::vector<std::string> &header, SimFields &f, std::vector<SimTag> &tags) {
  header = {"@SQ\tSN:chr1\tLN:12", "@SQ\tSN:chr2\tLN:12",
            "@PG\tID:epialleleR\tPN:epialleleR\tVN:1.13.4\tCL:rcpp_simulate_bam()"};
  f.qname = {"a", "bb", "ccc"};
  f.flag = {0, 16, 4};
  f.tid = {0, 1, 0};
  f.pos = {0, 4, 8};
  f.mapq = {60, 30, 0};
  f.cigar = {"4M", "2M1I1M", "*"};
  f.mtid = {0, 1, 0};
  f.mpos = {0, 0, 0};
  f.isize = {4, -4, 0};
  f.seq = {"ACGT", "acgn", "TTTT"};
  f.qual = {"FFFF", "!!!!", "IIII"};
  SimTag nm; nm.name = "NM"; nm.group = 'i'; nm.i = {1, -200, 70000};
  SimTag xf; xf.name = "XF"; xf.group = 'f'; xf.f = {0.5, -1.25, 0.1};
  SimTag xm; xm.name = "XM"; xm.group = 's'; xm.s = {"zZ..", "....", ""};
  SimTag ml; ml.name = "ML"; ml.group = 'a'; ml.type = 'C'; ml.a = {{1, 2}, {255}, {}};
  SimTag mf; mf.name = "MF"; mf.group = 'a'; mf.type = 'f'; mf.a = {{1.5}, {}, {-2.0, 0.25}};
  tags = {nm, xf, xm, ml, mf};
}

static int run_cpu() {
  std::vector<std::string> header;
  SimFields f;
  std::vector<SimTag> tags;
  shim_case(header, f, tags);
  SimColumns c;
  sim_columns(f, tags, c);
  EXPECT(c.nrecs == 3 && c.fields.size() == EPI_SIM_NFIELDS && c.tags.size() == 5);
  for (const epi_sim_column &col : c.fields) EXPECT(col.len == 3 && col.period == 3 && col.kind != EPI_SIM_NONE);
  EXPECT(c.fields[0].kind == EPI_SIM_STR && c.fields[0].offsets[3] == 6 && !memcmp(c.fields[0].values, "abbccc", 6));
  EXPECT(c.fields[3].kind == EPI_SIM_I32 && ((const int32_t *)c.fields[3].values)[2] == 8);
  EXPECT(c.fields[9].kind == EPI_SIM_STR && c.fields[10].kind == EPI_SIM_STR);
  EXPECT(!strcmp(c.tags[0].name, "NM") && c.tags[0].kind == EPI_SIM_I32 && ((const int32_t *)c.tags[0].values)[1] == -200);
  EXPECT(c.tags[1].kind == EPI_SIM_F32 && ((const float *)c.tags[1].values)[1] == -1.25f);
  EXPECT(c.tags[2].kind == EPI_SIM_STR && c.tags[2].offsets[3] == 8);
  EXPECT(c.tags[3].kind == EPI_SIM_ARR && c.tags[3].type == 'C' && c.tags[3].offsets[1] == 2 && c.tags[3].offsets[3] == 3 &&
         ((const int32_t *)c.tags[3].values)[2] == 255);
  EXPECT(c.tags[4].kind == EPI_SIM_ARR && c.tags[4].type == 'f' && ((const float *)c.tags[4].values)[2] == 0.25f);
  SimFields bad = f;
  bad.flag.pop_back();
  bool thrown = false;
  try { sim_columns(bad, tags, c); } catch (const std::exception &) { thrown = true; }
  EXPECT(thrown);
  bad = f;
  bad.pos[0] = 1LL << 31;
  thrown = false;
  try { sim_columns(bad, tags, c); } catch (const std::exception &e) { thrown = strstr(e.what(), "too large") != nullptr; }
  EXPECT(thrown);
  printf("shim simulate cpu ok\n");
  return 0;
}

static int run_gpu(const std::string &out) {
  std::vector<std::string> header;
  SimFields f;
  std::vector<SimTag> tags;
  shim_case(header, f, tags);
  EXPECT(simulate_bam(header, f, tags, out, 0, 2) == 3);
  SimFields bad = f;
  bad.cigar[1] = "2M1Q";
  bool thrown = false;
  try { simulate_bam(header, bad, tags, out + ".bad"); }
  catch (const std::exception &e) { thrown = strstr(e.what(), "Unable to fill CIGAR array") != nullptr; }
  EXPECT(thrown);
  printf("shim simulate gpu ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  try {
    if (!strcmp(argv[1], "cpu")) return run_cpu();
    if (!strcmp(argv[1], "gpu") && argc >= 3) return run_gpu(argv[2]);
  } catch (const std::exception &e) {
    fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  return 2;
}
