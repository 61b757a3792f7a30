// epi_preprocess_bam as a program of its own, for the host-only build of the library's host sources under the sanitizers
// (csrc/Makefile: make bam-host-test; tests/test_bam_host_sanitized.py runs it):
//
//     bam_host_main FILE [option=value ...]
//
// The options are the fields of epi_bam_options, on top of preprocessBam's defaults.  Standard output carries the outcome
// in a form to compare byte for byte: "error <code> <text>\n", or
// "ok n=<n> nbytes=<nbytes> nrecs=<nrecs> npushed=<n> paired=<0|1> targets=<name,...>\n" followed by the raw bytes of the
// five columns xm[nbytes], off[n + 1], rname[n], strand[n], start[n].  Exit status 0 either way; a sanitizer report ends
// the program with a status of its own.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/epihip.h"

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s FILE [option=value ...]\n", argv[0]); return 2; }
  epi_bam_options opt;
  memset(&opt, 0, sizeof(opt));
  opt.skip_secondary = opt.skip_qcfail = opt.skip_supplementary = 1;
  opt.paired = -1; opt.nthreads = 1; opt.min_prob = -1; opt.highest_prob = 1;
  const struct { const char *name; int32_t *v; } fields[] = {
      {"min_mapq", &opt.min_mapq}, {"min_baseq", &opt.min_baseq}, {"skip_duplicates", &opt.skip_duplicates},
      {"skip_secondary", &opt.skip_secondary}, {"skip_qcfail", &opt.skip_qcfail}, {"skip_supplementary", &opt.skip_supplementary},
      {"trim5", &opt.trim5}, {"trim3", &opt.trim3}, {"paired", &opt.paired}, {"nthreads", &opt.nthreads},
      {"min_prob", &opt.min_prob}, {"highest_prob", &opt.highest_prob}, {"window_kib", &opt.window_kib}};
  for (int a = 2; a < argc; a++) {
    const char *eq = strchr(argv[a], '=');
    bool known = false;
    for (const auto &f : fields)
      if (eq && strlen(f.name) == (size_t)(eq - argv[a]) && strncmp(f.name, argv[a], (size_t)(eq - argv[a])) == 0) {
        *f.v = (int32_t)strtol(eq + 1, nullptr, 10);
        known = true;
      }
    if (!known) { fprintf(stderr, "%s: unknown option %s\n", argv[0], argv[a]); return 2; }
  }
  epi_templates t;
  const int rc = epi_preprocess_bam(argv[1], &opt, &t);
  if (rc != EPI_OK) {
    printf("error %d %s\n", rc, epi_last_error());
    return 0;
  }
  printf("ok n=%lld nbytes=%lld nrecs=%lld npushed=%lld paired=%d targets=", (long long)t.n, (long long)t.nbytes,
         (long long)t.nrecs, (long long)t.n, (int)t.paired);
  for (int32_t i = 0; i < t.n_targets; i++) printf("%s%s", i ? "," : "", t.target_names[i]);
  printf("\n");
  const size_t n = (size_t)t.n;
  fwrite(t.xm, 1, (size_t)t.nbytes, stdout);
  fwrite(t.off, sizeof(int64_t), n + 1, stdout);
  fwrite(t.rname, sizeof(int32_t), n, stdout);
  fwrite(t.strand, sizeof(int32_t), n, stdout);
  fwrite(t.start, sizeof(int32_t), n, stdout);
  epi_templates_free(&t);
  return 0;
}
