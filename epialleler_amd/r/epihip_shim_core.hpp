// The SEXP-free half of the Rcpp shim (epihip_shim.cpp): everything between R's objects and the C ABI of
// libepihip.so that does not need Rcpp -- so it can be compiled and tested without R (tests/cpp/test_shim_core.cpp).
//
//  * gather_rows        std::vector<std::string> behind seqxm_xptr + templid  ->  one byte stream + offsets, row order
//  * Resident           what the new attribute `seqxm_hip_xptr` points at: the batch in HBM, uploaded ONCE per
//                       preprocessBam() object and reused by every later call (threshold -> cx without re-upload)
//  * bam_options        .readBam's arguments (R/internal.R:154-199: skip.flags as a sum) -> epi_bam_options
//  * materialize        SoA -> std::vector<std::string> for the out-of-scope functions that still read seqxm_xptr
//                       (rcpp_extract_patterns, rcpp_match_*, rcpp_get_base_freqs)
//  * gather_soa, RowOrder  the same row semantics for the producer's SoA, and the staleness check of the cached batch
//  * *_report_into      the report tables copied straight into columns the caller owns (R vectors): one D2H copy
//  * table guards       epi_cx_table / epi_mhl_table of the one-call entry points stay library-owned until freed
//  * base_freqs_into    rcpp_get_base_freqs: gathered rows + VCF sites -> the nsite x 20 matrix in the caller's memory
//  * fep_into           rcpp_fep: four count columns (R integers, or doubles with NA) -> two-sided p-values
//  * GenomeGuard, read_genome_into   rcpp_read_genome: the FASTA file -> rid / rname / rlen and the epi_genome the list's
//                       `rseq_xptr` owns
//  * call_methylation   rcpp_call_methylation_genome: BAM in, BAM out, with the strand tag R chose
//  * SimColumns, simulate_bam   rcpp_simulate_bam: the data.frames R has recycled to nrecs -> epi_sim_column (len =
//                       period = nrecs), the records assembled on the GPU
#pragma once
#include <stdint.h>
#include <string.h>
#include <cmath>
#include <stdexcept>
#include <type_traits>
#include <string>
#include <vector>
#include "epihip.h"

namespace epihip_shim {

struct Soa {
  std::vector<uint8_t> xm;
  std::vector<int64_t> off;
};

// row x is seqxm.at(templid[x]) (src/rcpp_cx_report.cpp:119); `poll` is called every 2^20 rows (interrupt check)
template <class Poll>
inline void gather_rows(const std::vector<std::string> &seqxm, const int32_t *templid, int64_t n, Soa &s, Poll poll) {
  s.off.resize((size_t)n + 1);
  int64_t total = 0;
  for (int64_t x = 0; x < n; x++) { s.off[(size_t)x] = total; total += (int64_t)seqxm.at((size_t)templid[x]).size(); }
  s.off[(size_t)n] = total;
  s.xm.resize((size_t)total + 16);
  for (int64_t x = 0; x < n; x++) {
    const std::string &t = seqxm[(size_t)templid[x]];
    if (!t.empty()) memcpy(s.xm.data() + s.off[(size_t)x], t.data(), t.size());
    if ((x & 0xFFFFF) == 0) poll();
  }
}

// The same for a table that still has the producer's SoA behind `seqxm_soa_xptr`: row x is template templid[x] of the
// producer's batch (what seqxm->at(templid[x]) means for the reference), so a table that was re-ordered by reference
// (setorder / setkey keep attributes), subset, or holds a template twice is served like the reference serves it.
template <class Poll>
inline void gather_soa(const epi_templates &t, const int32_t *templid, int64_t n, Soa &s, Poll poll) {
  s.off.resize((size_t)n + 1);
  int64_t total = 0;
  for (int64_t x = 0; x < n; x++) {
    const int64_t id = templid[x];
    if (id < 0 || id >= t.n) throw std::out_of_range("templid outside the preprocessed templates");   // vector::at
    s.off[(size_t)x] = total;
    total += t.off[id + 1] - t.off[id];
  }
  s.off[(size_t)n] = total;
  s.xm.resize((size_t)total + 16);
  for (int64_t x = 0; x < n; x++) {
    const int64_t id = templid[x], len = t.off[id + 1] - t.off[id];
    if (len > 0) memcpy(s.xm.data() + s.off[(size_t)x], t.xm + t.off[id], (size_t)len);
    if ((x & 0xFFFFF) == 0) poll();
  }
}

// What a resident batch was built from: the row count and the `templid` column (identity 0..n-1, or a hash of it).  A
// cached handle is reused only while the data.frame still has exactly this row order (a by-reference setorder or a subset
// that kept the attributes changes it).
struct RowOrder {
  int64_t n = -1;
  bool identity = false;
  uint64_t hash = 0;
  bool operator==(const RowOrder &o) const { return n == o.n && identity == o.identity && hash == o.hash; }
  bool operator!=(const RowOrder &o) const { return !(*this == o); }
};
inline RowOrder row_order_of(const int32_t *templid, int64_t n) {
  RowOrder r;
  r.n = n;
  r.identity = true;
  int64_t x = 0;
  for (; x < n; x++) if (templid[x] != (int32_t)x) { r.identity = false; break; }
  if (!r.identity) {
    uint64_t h = 1469598103934665603ull;                   // FNV-1a over the column
    for (x = 0; x < n; x++) { h ^= (uint32_t)templid[x]; h *= 1099511628211ull; }
    r.hash = h;
  }
  return r;
}

inline void check(int rc) {                      // the Rcpp shim turns this into Rcpp::stop (BEGIN_RCPP / END_RCPP)
  if (rc != EPI_OK) throw std::runtime_error(epi_last_error());
}

// The batch of one preprocessBam() object, resident in HBM.  Owned by an R external pointer (finalizer = delete).
struct Resident {
  epi_batch *batch = nullptr;
  int64_t n = 0;
  RowOrder order;                                  // the table rows this batch was uploaded from
  Resident() = default;
  Resident(const Resident &) = delete;
  Resident &operator=(const Resident &) = delete;
  ~Resident() { if (batch) epi_batch_free(batch); }

  // host SoA (gathered strings, or the producer's pinned buffers) -> HBM, once
  static Resident *upload(const uint8_t *xm, const int64_t *off, const int32_t *rname, const int32_t *strand,
                          const int32_t *start, int64_t n) {
    epi_engine *eng = nullptr;
    check(epi_default_engine(&eng));
    Resident *r = new Resident();
    const int rc = epi_batch_upload(eng, xm, off, rname, strand, start, n, &r->batch);
    if (rc != EPI_OK) { delete r; check(rc); }
    r->n = n;
    return r;
  }
};

// The report tables straight into columns the caller owns (R's IntegerVector / NumericVector): `alloc(nrow)` is called
// once the row count is known and returns the destinations.  One device-to-host copy, no library-owned table in between
// (the reference fills its vectors in place too, src/rcpp_cx_report.cpp:133-140).
template <class Alloc6>
inline int64_t cx_report_into(epi_batch *b, const int32_t *pass, const char *ctx, Alloc6 alloc) {
  int64_t nrow = 0;
  check(epi_batch_cx_report_begin(b, pass, ctx, &nrow));
  int32_t *cols[6];
  alloc(nrow, cols);
  if (nrow > 0) check(epi_batch_cx_fetch_host(b, cols, nullptr));
  return nrow;
}
template <class Alloc6>
inline int64_t cytosine_report_into(epi_batch *b, const char *ctx_meth, const char *ctx_unmeth, const char *ooctx_meth,
                                    const char *ooctx_unmeth, uint32_t min_n_ctx, double min_ctx_meth_frac,
                                    double max_ooctx_meth_frac, const char *ctx, int32_t *pass_out, Alloc6 alloc) {
  int64_t nrow = 0;
  check(epi_batch_cytosine_report_begin(b, ctx_meth, ctx_unmeth, ooctx_meth, ooctx_unmeth, min_n_ctx, min_ctx_meth_frac,
                                        max_ooctx_meth_frac, ctx, pass_out, &nrow));
  int32_t *cols[6];
  alloc(nrow, cols);
  if (nrow > 0) check(epi_batch_cx_fetch_host(b, cols, nullptr));
  return nrow;
}
template <class Alloc7>
inline int64_t mhl_report_into(epi_batch *b, const char *ctx, int hmax, int hmin, double max_ooctx_meth_frac, Alloc7 alloc) {
  int64_t nrow = 0;
  check(epi_batch_mhl_report_begin(b, ctx, hmax, hmin, max_ooctx_meth_frac, &nrow));
  int32_t *ic[5];
  double *dc[2];
  alloc(nrow, ic, dc);
  if (nrow > 0) check(epi_batch_mhl_fetch_host(b, ic, dc, nullptr));
  return nrow;
}

// .readBam's numeric arguments -> epi_bam_options (skip.flags = 4 [+256] [+512] [+1024] [+2048] [+8 when paired])
inline epi_bam_options bam_options(int min_mapq, int min_baseq, int skip_flags, int trim5, int trim3, int nthreads,
                                   int paired, int min_prob = -1, bool highest_prob = true) {
  epi_bam_options o;
  memset(&o, 0, sizeof(o));
  o.min_mapq = min_mapq;
  o.min_baseq = min_baseq;
  o.skip_secondary = (skip_flags & 256) != 0;
  o.skip_qcfail = (skip_flags & 512) != 0;
  o.skip_duplicates = (skip_flags & 1024) != 0;
  o.skip_supplementary = (skip_flags & 2048) != 0;
  o.trim5 = trim5;
  o.trim3 = trim3;
  o.paired = paired;
  o.nthreads = nthreads < 1 ? 1 : nthreads;
  o.min_prob = min_prob;
  o.highest_prob = highest_prob ? 1 : 0;
  return o;
}

// the std::vector<std::string> view of a producer batch (rows are already in (rname,start) order: templid = 0..n-1)
inline void materialize(const epi_templates &t, std::vector<std::string> &seqxm) {
  seqxm.clear();
  seqxm.reserve((size_t)t.n);
  for (int64_t x = 0; x < t.n; x++)
    seqxm.emplace_back(reinterpret_cast<const char *>(t.xm) + t.off[x], (size_t)(t.off[x + 1] - t.off[x]));
}

// frees a library-owned table when it goes out of scope (also when copying into R vectors throws)
struct CxTableGuard {
  epi_cx_table t;
  CxTableGuard() { memset(&t, 0, sizeof(t)); }
  ~CxTableGuard() { epi_cx_table_free(&t); }
};
struct MhlTableGuard {
  epi_mhl_table t;
  MhlTableGuard() { memset(&t, 0, sizeof(t)); }
  ~MhlTableGuard() { epi_mhl_table_free(&t); }
};
struct TemplatesGuard {                       // owner behind `seqxm_soa_xptr`
  epi_templates t;
  TemplatesGuard() { memset(&t, 0, sizeof(t)); }
  TemplatesGuard(const TemplatesGuard &) = delete;
  TemplatesGuard &operator=(const TemplatesGuard &) = delete;
  ~TemplatesGuard() { epi_templates_free(&t); }
};

// rcpp_get_base_freqs (src/rcpp_get_base_freqs.cpp:15-57): `out` is the column-major nsite x 20 NumericMatrix.  pass as R
// logicals (NULL = all TRUE); vcf_chr are factor codes over the BAM's rname levels (NA_integer_ = INT32_MIN: zero row).
inline void base_freqs_into(const Soa &s, const int32_t *rname, const int32_t *strand, const int32_t *start, int64_t n,
                            const int32_t *pass, const int32_t *vcf_chr, const int32_t *vcf_pos, int64_t nsite, double *out) {
  check(epi_get_base_freqs(s.xm.data(), s.off.data(), n, rname, strand, start, pass, vcf_chr, vcf_pos, nsite, out));
}

// rcpp_fep (src/rcpp_fep.cpp:10-36) over columns of any numeric type: NA (INT32_MIN, or NaN in a double column) in any
// cell gives NaN (NA_real_)
template <class T>
inline void fep_into(const T *a, const T *b, const T *c, const T *d, int64_t n, double *out, int nthreads = 1) {
  std::vector<int32_t> v[4];
  const T *src[4] = {a, b, c, d};
  for (int k = 0; k < 4; k++) {
    v[k].resize((size_t)n);
    for (int64_t i = 0; i < n; i++) {
      const T x = src[k][i];
      bool na = false;
      if constexpr (std::is_floating_point<T>::value) na = std::isnan(x);
      v[k][(size_t)i] = na ? INT32_MIN : (int32_t)x;
    }
  }
  check(epi_fisher_exact(v[0].data(), v[1].data(), v[2].data(), v[3].data(), n, out, nthreads));
}

// rcpp_read_genome (src/rcpp_read_genome.cpp:50-98): the sequences stay in the library; the list's rseq_xptr owns them
struct GenomeGuard {
  epi_genome *g = nullptr;
  GenomeGuard() = default;
  GenomeGuard(const GenomeGuard &) = delete;
  GenomeGuard &operator=(const GenomeGuard &) = delete;
  ~GenomeGuard() { epi_genome_free(g); }
};
inline void read_genome_into(const std::string &fn, int nthreads, GenomeGuard &gg, std::vector<uint64_t> &rid,
                             std::vector<std::string> &rname, std::vector<uint64_t> &rlen) {
  epi_genome_free(gg.g);
  gg.g = nullptr;
  check(epi_read_genome(fn.c_str(), nthreads > 0 ? nthreads : 1, &gg.g));
  const int32_t n = epi_genome_count(gg.g);
  rid.resize((size_t)n); rname.resize((size_t)n); rlen.resize((size_t)n);
  for (int32_t i = 0; i < n; i++) {
    rid[(size_t)i] = (uint64_t)i;
    rname[(size_t)i] = epi_genome_name(gg.g, i);
    rlen[(size_t)i] = (uint64_t)epi_genome_length(gg.g, i);
  }
}

// rcpp_call_methylation_genome (src/rcpp_call_methylation.cpp:27-177): `tag` is what .callMethylation chose (XG/YD/ZS);
// the default engine's device does the calls
inline void call_methylation(const std::string &in_fn, const std::string &out_fn, const GenomeGuard &gg, const std::string &tag,
                             int nthreads, int64_t *nrecs, int64_t *ncalled) {
  if (!gg.g) throw std::runtime_error("genome object has no sequences attached");
  check(epi_call_methylation_windowed(nullptr, in_fn.c_str(), out_fn.c_str(), gg.g, tag.c_str(), nthreads > 0 ? nthreads : 1, 0,
                                      nrecs, ncalled));
}

// rcpp_simulate_bam (src/rcpp_simulate_bam.cpp): .simulateBam has recycled every column to nrecs, so each one is shipped
// with len = period = nrecs.  The column structs point into the vectors held here.
struct SimTag {
  std::string name;
  char group = 'i';                      // 'i' (integer), 'f' (float), 's' (string), 'a' (array)
  char type = 0;                         // arrays: the subtype R chose (a_types), c C s S i I f
  std::vector<int32_t> i;
  std::vector<double> f;
  std::vector<std::string> s;
  std::vector<std::vector<double>> a;
};
struct SimFields {
  std::vector<std::string> qname, cigar, seq, qual;
  std::vector<int32_t> flag, tid, mapq, mtid;
  std::vector<int64_t> pos, mpos, isize;   // hts_pos_t in the reference
};
struct SimColumns {
  std::vector<epi_sim_column> fields, tags;
  std::vector<std::vector<int32_t>> i32;
  std::vector<std::vector<float>> f32;
  std::vector<std::vector<char>> bytes;
  std::vector<std::vector<int64_t>> offs;
  int64_t nrecs = 0;
};
inline void sim_strings(SimColumns &c, const std::vector<std::string> &v, epi_sim_column &col) {
  std::vector<char> b;
  std::vector<int64_t> o(1, 0);
  for (const std::string &x : v) { b.insert(b.end(), x.begin(), x.end()); o.push_back((int64_t)b.size()); }
  b.push_back(0);
  c.bytes.push_back(std::move(b));
  c.offs.push_back(std::move(o));
  col.kind = EPI_SIM_STR;
  col.values = c.bytes.back().data();
  col.offsets = c.offs.back().data();
}
inline void sim_ints(SimColumns &c, std::vector<int32_t> v, epi_sim_column &col) {
  c.i32.push_back(std::move(v));
  col.kind = EPI_SIM_I32;
  col.values = c.i32.back().data();
}
inline std::vector<int32_t> sim_narrow(const std::vector<int64_t> &v, const char *what) {
  std::vector<int32_t> r(v.size());
  for (size_t k = 0; k < v.size(); k++) {
    if (v[k] < INT32_MIN || v[k] > INT32_MAX) throw std::runtime_error(std::string("Positional data is too large for BAM format: ") + what);
    r[k] = (int32_t)v[k];
  }
  return r;
}
inline void sim_columns(const SimFields &f, const std::vector<SimTag> &tags, SimColumns &c) {
  const size_t n = f.qname.size();
  const std::vector<size_t> lens = {f.flag.size(), f.tid.size(), f.pos.size(), f.mapq.size(), f.cigar.size(),
                                    f.mtid.size(), f.mpos.size(), f.isize.size(), f.seq.size(), f.qual.size()};
  for (size_t l : lens)
    if (l != n) throw std::runtime_error("rcpp_simulate_bam: the fields differ in length");
  c = SimColumns();
  c.nrecs = (int64_t)n;
  const size_t ncol = 2 * (EPI_SIM_NFIELDS + tags.size()) + 8;   // reserved: the structs point into these vectors
  c.i32.reserve(ncol); c.f32.reserve(ncol); c.bytes.reserve(ncol); c.offs.reserve(ncol);
  c.fields.assign(EPI_SIM_NFIELDS, epi_sim_column());
  for (epi_sim_column &col : c.fields) { memset(&col, 0, sizeof(col)); col.len = col.period = (int64_t)(n ? n : 1); }
  sim_strings(c, f.qname, c.fields[0]);
  sim_ints(c, f.flag, c.fields[1]);
  sim_ints(c, f.tid, c.fields[2]);
  sim_ints(c, sim_narrow(f.pos, "pos"), c.fields[3]);
  sim_ints(c, f.mapq, c.fields[4]);
  sim_strings(c, f.cigar, c.fields[5]);
  sim_ints(c, f.mtid, c.fields[6]);
  sim_ints(c, sim_narrow(f.mpos, "mpos"), c.fields[7]);
  sim_ints(c, sim_narrow(f.isize, "isize"), c.fields[8]);
  sim_strings(c, f.seq, c.fields[9]);
  sim_strings(c, f.qual, c.fields[10]);
  c.tags.assign(tags.size(), epi_sim_column());
  for (size_t k = 0; k < tags.size(); k++) {
    const SimTag &t = tags[k];
    epi_sim_column &col = c.tags[k];
    memset(&col, 0, sizeof(col));
    col.name = t.name.c_str();
    col.len = col.period = (int64_t)(n ? n : 1);
    const size_t len = t.group == 'i' ? t.i.size() : t.group == 'f' ? t.f.size() : t.group == 's' ? t.s.size() : t.a.size();
    if (t.name.size() != 2 || len != n) throw std::runtime_error("rcpp_simulate_bam: bad tag column " + t.name);
    if (t.group == 'i') {
      sim_ints(c, t.i, col);
    } else if (t.group == 'f') {
      c.f32.emplace_back(t.f.begin(), t.f.end());            // bam_aux_update_float(float)
      col.kind = EPI_SIM_F32;
      col.values = c.f32.back().data();
    } else if (t.group == 's') {
      sim_strings(c, t.s, col);
    } else {
      if (!t.type || !strchr("cCsSiIf", t.type)) throw std::runtime_error("rcpp_simulate_bam: bad array type for " + t.name);
      std::vector<int64_t> o(1, 0);
      std::vector<int32_t> iv;
      std::vector<float> fv;
      for (const std::vector<double> &x : t.a) {
        for (double d : x) {                                   // save_array_tag: static_cast<T>(value)
          if (t.type == 'f') fv.push_back((float)d);
          else iv.push_back(t.type == 'I' ? (int32_t)(uint32_t)d : (int32_t)d);
        }
        o.push_back((int64_t)(t.type == 'f' ? fv.size() : iv.size()));
      }
      if (t.type == 'f') { fv.push_back(0.0f); c.f32.push_back(std::move(fv)); col.values = c.f32.back().data(); }
      else { iv.push_back(0); c.i32.push_back(std::move(iv)); col.values = c.i32.back().data(); }
      c.offs.push_back(std::move(o));
      col.kind = EPI_SIM_ARR;
      col.type = t.type;
      col.offsets = c.offs.back().data();
    }
  }
}
// the default engine's device assembles the records; returns the number written
inline int64_t simulate_bam(const std::vector<std::string> &header, const SimFields &f, const std::vector<SimTag> &tags,
                            const std::string &out_fn, uint64_t seed = 0, int nthreads = 1) {
  SimColumns c;
  sim_columns(f, tags, c);
  std::vector<const char *> lines;
  for (const std::string &h : header) lines.push_back(h.c_str());
  int64_t nw = 0;
  check(epi_simulate_bam(nullptr, out_fn.c_str(), lines.data(), (int32_t)lines.size(), c.nrecs, c.fields.data(),
                         c.tags.empty() ? nullptr : c.tags.data(), (int32_t)c.tags.size(), seed, nthreads, 0, &nw));
  return nw;
}

}  // namespace epihip_shim
