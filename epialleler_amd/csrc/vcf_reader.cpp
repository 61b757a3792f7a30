// VCF reader for generateVcfReport (what .readVcf gets from VariantAnnotation::readVcf(info = NA, geno = NA) followed by
// expand(), R/internal.R:230-267 and R/generateVcfReport.R): plain, gzip or BGZF text; the fixed columns only.
// Every record becomes one row per ALT allele; rows whose REF is not one base or whose ALT is not one character are
// dropped here, as .getBaseFreqReport does (R/internal.R:617-620).  Rows stay in file order.  Contigs are numbered in
// the order of the ##contig header lines, then in the order of first appearance (readVcf's seqlevels).
#include <stdlib.h>
#include <string.h>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>
#include "common.hpp"

using namespace epi;

namespace {

// ##contig=<ID=name,...>
bool contig_id(const char *p, const char *e, std::string *id) {
  static const char kTag[] = "##contig=<";
  const size_t lt = sizeof(kTag) - 1;
  if ((size_t)(e - p) < lt || memcmp(p, kTag, lt) != 0) return false;
  for (const char *q = p + lt; q + 3 <= e; q++) {
    if ((q == p + lt || q[-1] == ',') && memcmp(q, "ID=", 3) == 0) {
      const char *s = q + 3, *t = s;
      while (t < e && *t != ',' && *t != '>') t++;
      id->assign(s, t);
      return !id->empty();
    }
  }
  return false;
}

}  // namespace

extern "C" int epi_read_vcf(const char *path, epi_vcf *out) {
  if (!out) return fail(EPI_ERR_ARG, "epi_read_vcf: out is NULL");
  memset(out, 0, sizeof(*out));
  if (!path) return fail(EPI_ERR_ARG, "epi_read_vcf: path is NULL");
  std::vector<uint8_t> text;
  const unsigned hw = std::thread::hardware_concurrency();
  EPI_TRY(read_text_file(path, text, hw > 16 ? 16 : (hw ? (int)hw : 1)));
  std::vector<std::string> names;
  std::unordered_map<std::string, int32_t> index;
  auto chrom_of = [&](const std::string &s) {
    auto it = index.find(s);
    if (it != index.end()) return it->second;
    const int32_t k = (int32_t)names.size();
    names.push_back(s);
    index.emplace(s, k);
    return k;
  };
  std::vector<int32_t> chrom, pos;
  std::vector<char> ref, alt, nm;
  int64_t nfile = 0;
  bool header_done = false;
  const char *p = reinterpret_cast<const char *>(text.data()), *end = p + text.size();
  std::string tmp, id;
  int64_t line_no = 0;
  while (p < end) {
    const char *e = static_cast<const char *>(memchr(p, '\n', (size_t)(end - p)));
    if (!e) e = end;
    const char *le = (e > p && e[-1] == '\r') ? e - 1 : e;
    line_no++;
    if (le == p) { p = e + 1; continue; }
    if (*p == '#') {
      if (!header_done && contig_id(p, le, &tmp)) chrom_of(tmp);
      p = e + 1;
      continue;
    }
    header_done = true;
    const char *f[6];                              // CHROM POS ID REF ALT and the end of ALT
    int nf = 0;
    const char *q = p;
    f[nf++] = q;
    while (q < le && nf < 6) { if (*q == '\t') f[nf++] = q + 1; q++; }
    if (nf < 5) return fail(EPI_ERR_ARG, "VCF line %lld: fewer than 5 tab-separated fields", (long long)line_no);
    const char *alt_end = nf == 6 ? f[5] - 1 : le;
    nfile++;
    tmp.assign(f[0], f[1] - 1);
    const int32_t c = chrom_of(tmp);
    char *pe = nullptr;
    const long long ps = strtoll(f[1], &pe, 10);
    if (pe == f[1] || ps < INT32_MIN || ps > INT32_MAX)
      return fail(EPI_ERR_ARG, "VCF line %lld: bad POS", (long long)line_no);
    const char *r0 = f[3], *r1 = f[4] - 1;
    if (r1 - r0 != 1) { p = e + 1; continue; }     // REF of more than one base: width(rowRanges) != 1
    // name: ID, or CHROM:POS_REF/ALT when it is "." (VariantAnnotation's row names)
    const bool no_id = f[2][0] == '.' && f[3] - 1 == f[2] + 1;
    if (no_id) {
      id.assign(f[0], f[1] - 1);
      id += ':';
      id.append(f[1], f[2] - 1);
      id += '_';
      id.append(r0, r1);
      id += '/';
      id.append(f[4], alt_end);
    } else {
      id.assign(f[2], f[3] - 1);
    }
    for (const char *a = f[4]; a <= alt_end;) {    // one row per ALT allele
      const char *z = a;
      while (z < alt_end && *z != ',') z++;
      if (z - a == 1 && *a != '.') {               // single-character ALT ("." is no allele)
        chrom.push_back(c);
        pos.push_back((int32_t)ps);
        ref.push_back(*r0);
        alt.push_back(*a);
        nm.insert(nm.end(), id.begin(), id.end());
        nm.push_back('\0');
      }
      a = z + 1;
    }
    p = e + 1;
  }
  const size_t m = chrom.size();
  const size_t nb = m ? m : 1;
  out->chrom = static_cast<int32_t *>(malloc(nb * 4));
  out->pos = static_cast<int32_t *>(malloc(nb * 4));
  out->ref = static_cast<char *>(malloc(nb));
  out->alt = static_cast<char *>(malloc(nb));
  out->names = static_cast<char *>(malloc(nm.size() + 1));
  out->chrom_names = static_cast<char **>(calloc(names.size() + 1, sizeof(char *)));
  if (!out->chrom || !out->pos || !out->ref || !out->alt || !out->names || !out->chrom_names) {
    epi_vcf_free(out);
    return fail(EPI_ERR_NOMEM, "out of host memory for the VCF table");
  }
  if (m) {
    memcpy(out->chrom, chrom.data(), m * 4);
    memcpy(out->pos, pos.data(), m * 4);
    memcpy(out->ref, ref.data(), m);
    memcpy(out->alt, alt.data(), m);
  }
  if (!nm.empty()) memcpy(out->names, nm.data(), nm.size());
  out->names[nm.size()] = '\0';
  for (size_t i = 0; i < names.size(); i++) out->chrom_names[i] = strdup(names[i].c_str());
  out->nrec = (int64_t)m;
  out->nrec_file = nfile;
  out->names_bytes = (int64_t)nm.size();
  out->n_chrom = (int32_t)names.size();
  return EPI_OK;
}

extern "C" void epi_vcf_free(epi_vcf *v) {
  if (!v) return;
  if (v->chrom_names)
    for (int32_t i = 0; i < v->n_chrom; i++) free(v->chrom_names[i]);
  free(v->chrom_names);
  free(v->chrom); free(v->pos); free(v->ref); free(v->alt); free(v->names);
  memset(v, 0, sizeof(*v));
}
