// Reference genome for callMethylation (what rcpp_read_genome, src/rcpp_read_genome.cpp:50-98, keeps behind the
// genome list's rseq_xptr): the sequences of a FASTA file, in file order, as one contiguous byte array plus per-contig
// offsets.  No .fai index: the whole file is read through read_text_file (plain, gzip or BGZF) and split at the header
// lines.  Like faidx, a name is the header up to the first whitespace and only printable non-space bytes of the
// sequence lines count as bases; every base other than aAcCgGtTnN becomes 'N', lower case becomes upper case.
//
// The bytes are uploaded to a device the first time a call there needs them (genome_device) and stay resident until the
// object is freed: a genome is read once and serves every later callMethylation.
#include <ctype.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <string>
#include <unordered_set>
#include <vector>
#include "common.hpp"

using namespace epi;

struct epi_genome {
  std::vector<std::string> names;
  std::vector<int64_t> off;          // contig i owns seq[off[i], off[i + 1])
  std::vector<char> seq;             // 'A' 'C' 'G' 'T' 'N' only
  std::mutex mu;                     // guards the device copies
  struct Dev { int device; uint8_t *seq; int64_t *off; };
  std::vector<Dev> dev;
  ~epi_genome() {
#ifndef EPI_HOST_ONLY
    for (const Dev &d : dev) {
      int cur = -1;
      (void)hipGetDevice(&cur);
      if (hipSetDevice(d.device) == hipSuccess) { (void)hipFree(d.seq); (void)hipFree(d.off); }
      if (cur >= 0) (void)hipSetDevice(cur);
      (void)hipGetLastError();
    }
#endif
  }
};

namespace {

// 'A' 'C' 'G' 'T' 'N' for a (printable) FASTA byte
struct BaseFilter {
  char t[256];
  BaseFilter() {
    for (int c = 0; c < 256; c++) t[c] = 'N';
    for (const char *p = "ACGT"; *p; p++) { t[(unsigned char)*p] = *p; t[(unsigned char)tolower(*p)] = *p; }
  }
};
const BaseFilter kFilter;

}  // namespace

namespace epi {

int genome_device(epi_genome *g, int device, const uint8_t **d_seq, const int64_t **d_off) {
#ifdef EPI_HOST_ONLY
  (void)g; (void)device; (void)d_seq; (void)d_off;
  return fail(EPI_ERR_NODEVICE, "host-only build: no device");
#else
  std::lock_guard<std::mutex> lk(g->mu);
  for (const epi_genome::Dev &d : g->dev)
    if (d.device == device) { *d_seq = d.seq; *d_off = d.off; return EPI_OK; }
  EPI_HIP(hipSetDevice(device));
  epi_genome::Dev d{device, nullptr, nullptr};
  // (+16: the halo reads of the kernel stay inside the contig, the padding only keeps an empty genome allocatable)
  EPI_HIP(hipMalloc(&d.seq, g->seq.size() + 16));
  if (hipMalloc(&d.off, g->off.size() * sizeof(int64_t)) != hipSuccess) {
    (void)hipFree(d.seq); (void)hipGetLastError();
    return fail(EPI_ERR_NOMEM, "genome upload: out of device memory");
  }
  hipError_t e = hipMemcpy(d.seq, g->seq.data(), g->seq.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d.off, g->off.data(), g->off.size() * sizeof(int64_t), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(d.seq); (void)hipFree(d.off); (void)hipGetLastError();
    return fail(EPI_ERR_HIP, "genome upload failed: %s", hipGetErrorName(e));
  }
  g->dev.push_back(d);
  *d_seq = d.seq; *d_off = d.off;
  return EPI_OK;
#endif
}

}  // namespace epi

extern "C" {

int epi_read_genome(const char *path, int nthreads, epi_genome **out) {
  if (!out) return fail(EPI_ERR_ARG, "epi_read_genome: out is NULL");
  *out = nullptr;
  if (!path) return fail(EPI_ERR_ARG, "epi_read_genome: path is NULL");
  try {
    std::vector<uint8_t> text;
    if (read_text_file(path, text, nthreads > 0 ? nthreads : 1) != EPI_OK)
      return fail(EPI_ERR_ARG, "Unable to open FASTA file for reading: %s", path);
    epi_genome *g = new epi_genome();
    std::unique_ptr<epi_genome> guard(g);
    g->seq.reserve(text.size());
    std::unordered_set<std::string> seen;
    const uint8_t *p = text.data(), *e = text.data() + text.size();
    while (p < e) {
      const uint8_t *nl = static_cast<const uint8_t *>(memchr(p, '\n', (size_t)(e - p)));
      const uint8_t *le = nl ? nl : e;
      if (*p == '>') {
        const uint8_t *s = p + 1, *t = s;
        while (t < le && !isspace(*t)) t++;
        std::string name((const char *)s, (size_t)(t - s));
        if (name.empty()) return fail(EPI_ERR_ARG, "FASTA header without a sequence name in %s", path);
        if (!seen.insert(name).second) return fail(EPI_ERR_ARG, "duplicate sequence name in FASTA file: %s", name.c_str());
        g->names.push_back(std::move(name));
        g->off.push_back((int64_t)g->seq.size());
      } else {
        for (const uint8_t *q = p; q < le; q++) {
          if (!isgraph(*q)) continue;                      // blanks, '\r', an empty line
          if (g->names.empty()) return fail(EPI_ERR_ARG, "not a FASTA file (sequence before the first header): %s", path);
          g->seq.push_back(kFilter.t[*q]);
        }
      }
      p = le + 1;
    }
    if (g->names.empty()) return fail(EPI_ERR_ARG, "no sequences in FASTA file %s", path);
    g->off.push_back((int64_t)g->seq.size());
    *out = guard.release();
    return EPI_OK;
  } catch (const std::bad_alloc &) {
    return fail(EPI_ERR_NOMEM, "epi_read_genome: out of host memory");
  }
}

void epi_genome_free(epi_genome *g) { delete g; }

int32_t epi_genome_count(const epi_genome *g) { return g ? (int32_t)g->names.size() : 0; }

const char *epi_genome_name(const epi_genome *g, int32_t i) {
  return g && i >= 0 && (size_t)i < g->names.size() ? g->names[(size_t)i].c_str() : nullptr;
}

int64_t epi_genome_length(const epi_genome *g, int32_t i) {
  return g && i >= 0 && (size_t)i < g->names.size() ? g->off[(size_t)i + 1] - g->off[(size_t)i] : -1;
}

const char *epi_genome_sequence(const epi_genome *g, int32_t i) {
  return g && i >= 0 && (size_t)i < g->names.size() ? g->seq.data() + g->off[(size_t)i] : nullptr;
}

}  // extern "C"
