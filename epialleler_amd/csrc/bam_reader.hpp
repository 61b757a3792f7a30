// The BAM reader: the BGZF and file layer, the thread fan-out of the host loops, one alignment record (Rec) with its aux
// walkers, and the file as windows of inflated, parsed records (BamWindows).  Pure host code: nothing here touches the
// device (bam_device.hpp has what does).  Used by the packers (bam_pack.cpp), callMethylation (bam_call.cpp) and, for the
// whole-file inflate, the text readers (read_text_file in common.hpp).  What is called per record or per base is inline
// here, and static: where the compiler does not inline a call, it stays a direct call inside the shared library (an inline
// function with external linkage is called through the PLT), as when all of this was one anonymous namespace.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <chrono>
#include <new>
#include <string>
#include <thread>
#include <vector>
#include "common.hpp"

namespace epi {
namespace bam {

// Large host buffers (the inflated window, the packed bytes of a thread, the record index): 2 MiB-aligned and advised
// as huge pages -- a first touch then faults 2 MiB at a time instead of 4 KiB (hundreds of thousands of faults per file
// from 16 threads otherwise).  Released with free().
static inline void *big_malloc(size_t bytes) {
  constexpr size_t HUGE = (size_t)2 << 20;
  if (bytes >= 4 * HUGE && !epi::options().no_hugepage) {
    const size_t r = (bytes + HUGE - 1) & ~(HUGE - 1);
    void *p = aligned_alloc(HUGE, r);
    if (p) { (void)madvise(p, r, MADV_HUGEPAGE); return p; }
  }
  return malloc(bytes);
}
static inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
static inline uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }

// ---- the BGZF and file layer -------------------------------------------------------------------------------------------
struct Block {
  size_t cpos, clen; size_t upos, ulen;                     // compressed payload / uncompressed placement
  // what the inflating thread found when it walked the block's bytes as a chain of BAM records starting at the block's
  // first byte: their number, and whether the chain ends exactly at the block's end.  (HTSlib never lets a record
  // straddle two blocks unless it is larger than one, so this is the true chain nearly always -- the index uses it
  // only where the true chain does arrive at the block's first byte.)
  uint32_t spec_n = 0;
  bool spec_ok = false;
};

// The compressed file, memory-mapped (read into a buffer where mmap is not possible): nothing of it is copied.
struct FileView {
  const uint8_t *p = nullptr;
  size_t n = 0;
  bool mapped = false;
  std::vector<uint8_t> own;
  ~FileView() { if (mapped && p) munmap(const_cast<uint8_t *>(p), n); }
};
int open_file(const char *path, FileView &v);
// Locate the BGZF blocks (no inflation).
int bgzf_scan(const uint8_t *in, size_t n, std::vector<Block> &blocks);
// Inflate blocks [b0, b1) to out + their upos, in parallel.
int bgzf_inflate_range(const uint8_t *in, std::vector<Block> &blocks, size_t b0, size_t b1, uint8_t *out, int nthreads);

// ---- the thread fan-out of the host loops ------------------------------------------------------------------------------
static inline double tnow() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the caller's nthreads -> threads of the host loops (the inflate takes nthreads as given)
static inline size_t thread_cap(int nthreads) { return nthreads > 1 ? (size_t)(nthreads > 16 ? 16 : nthreads) : 1; }

// [0, n) in K nearly equal ranges: the K + 1 cut points
static inline std::vector<size_t> even_cuts(size_t n, size_t K) {
  std::vector<size_t> cut(K + 1);
  for (size_t k = 0; k <= K; k++) cut[k] = n * k / K;
  return cut;
}

// Runs f(k, cut[k], cut[k + 1]) for every part k: part 0 here, the others on a thread each.  Nothing unwinds out of a
// thread, and the first part's error wins (by part, not by time; the message is thread-local, so each part keeps its own).
template <class F>
int fan_out(const std::vector<size_t> &cut, const char *who, const char *what, F &&f) {
  const size_t K = cut.size() - 1;
  std::vector<int> rcs(K, EPI_OK);
  std::vector<std::string> msgs(K);
  auto run = [&](size_t k) {
    try {
      rcs[k] = f(k, cut[k], cut[k + 1]);
    } catch (const std::bad_alloc &) {
      rcs[k] = fail(EPI_ERR_NOMEM, "%s: out of host memory", who);
    } catch (...) {
      rcs[k] = fail(EPI_ERR_ARG, "%s: unexpected failure while %s", who, what);
    }
    if (rcs[k] != EPI_OK) msgs[k] = epi_last_error();
  };
  std::vector<std::thread> th;
  for (size_t k = 1; k < K; k++) th.emplace_back(run, k);
  run(0);
  for (auto &t : th) t.join();
  for (size_t k = 0; k < K; k++)
    if (rcs[k] != EPI_OK) return fail(rcs[k], "%s", msgs[k].c_str());
  return EPI_OK;
}

// f(lo, hi) over K even ranges of [0, n) (one thread below 4096 items)
template <class F>
int parallel_ranges(size_t K, size_t n, const char *who, F &&f) {
  return fan_out(even_cuts(n, n < 4096 ? 1 : K), who, "processing records", [&](size_t, size_t lo, size_t hi) { return f(lo, hi); });
}

// ---- one record and its aux fields -------------------------------------------------------------------------------------
struct Rec {                 // one BAM alignment record, pointing into the inflated stream
  int32_t tid, pos, mtid, mpos, isize, l_seq;
  uint32_t n_cigar;
  uint16_t flag;
  uint8_t mapq;
  const char *qname;
  const uint8_t *cigar, *seq, *qual, *aux, *end;
};

// One record of the inflated stream -> Rec, with the structural checks HTSlib's bam_read1 makes (sizes consistent
// with block_size, NUL-terminated name); false: the record is not well-formed.
static inline bool parse_record(const uint8_t *b, uint32_t bs, Rec *r) {
  if (bs < 32) return false;
  r->tid = (int32_t)rd32(b); r->pos = (int32_t)rd32(b + 4);
  const uint32_t l_qname = b[8];
  r->mapq = b[9];
  r->n_cigar = rd16(b + 12); r->flag = rd16(b + 14);
  r->l_seq = (int32_t)rd32(b + 16); r->mtid = (int32_t)rd32(b + 20); r->mpos = (int32_t)rd32(b + 24); r->isize = (int32_t)rd32(b + 28);
  if (l_qname < 1 || r->l_seq < 0) return false;
  const uint64_t need = 32ull + l_qname + 4ull * r->n_cigar + ((uint64_t)r->l_seq + 1) / 2 + (uint64_t)r->l_seq;
  if (need > bs) return false;
  r->qname = (const char *)b + 32;
  if (b[32 + l_qname - 1] != 0) return false;
  r->cigar = b + 32 + l_qname;
  r->seq = r->cigar + 4 * (size_t)r->n_cigar;
  r->qual = r->seq + ((size_t)r->l_seq + 1) / 2;
  r->aux = r->qual + (size_t)r->l_seq;
  r->end = b + bs;
  return true;
}

// The aux field (tag, type, value: SAM spec 4.2.4) at p, p + 3 <= end: the byte after its value, or NULL where the field
// is malformed (a string without its NUL, an array header cut short, an unknown type).  Values of fixed size and array
// elements may run past `end`: the walkers below stop there by their loop condition.
static inline const uint8_t *aux_value_end(const uint8_t *p, const uint8_t *end) {
  const uint8_t *v = p + 3;
  switch ((char)p[2]) {
    case 'A': case 'c': case 'C': return v + 1;
    case 's': case 'S': return v + 2;
    case 'i': case 'I': case 'f': return v + 4;
    case 'Z': case 'H': {
      const uint8_t *e = (const uint8_t *)memchr(v, 0, (size_t)(end - v));
      return e ? e + 1 : nullptr;
    }
    case 'B': {
      if (v + 5 > end) return nullptr;
      const char sub = (char)v[0];
      const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
      return v + 5 + (size_t)rd32(v + 1) * es;
    }
    default: return nullptr;
  }
}

// bam_aux_get for Z-typed tags: pointer to the first character, or NULL.  *present: the tag is there (with a NULL
// result: not as a string).  A tag at or behind a malformed field is absent.
static inline const char *aux_z(const Rec &r, char a, char b, bool *present) {
  *present = false;
  for (const uint8_t *p = r.aux; p + 3 <= r.end;) {
    const uint8_t *next = aux_value_end(p, r.end);
    if (!next) return nullptr;
    if ((char)p[0] == a && (char)p[1] == b) {
      *present = true;
      return p[2] == 'Z' || p[2] == 'H' ? (const char *)p + 3 : nullptr;
    }
    p = next;
  }
  return nullptr;
}

static inline bool has_tag(const Rec &r, char a, char b) { bool pr; (void)aux_z(r, a, b, &pr); return pr; }

// bam_aux_get for B-typed (array) tags: element type, count and a pointer to the first element; false if absent.  Every
// array on the way, the tag's own included, must lie inside the record.
static inline bool aux_b(const Rec &r, char a, char b, char *sub, uint32_t *count, const uint8_t **data) {
  for (const uint8_t *p = r.aux; p + 3 <= r.end;) {
    const uint8_t *next = aux_value_end(p, r.end);
    if (!next || (p[2] == 'B' && next > r.end)) return false;
    if ((char)p[0] == a && (char)p[1] == b) {
      if (p[2] != 'B') return false;
      *sub = (char)p[3]; *count = rd32(p + 4); *data = p + 8;
      return true;
    }
    p = next;
  }
  return false;
}

// bam_aux_get: the tag's type byte, or NULL when the record has no such tag (or its aux data is malformed before it;
// the tag's own field is not looked at)
static inline const uint8_t *aux_find(const Rec &r, char a, char b) {
  for (const uint8_t *p = r.aux; p && p + 3 <= r.end; p = aux_value_end(p, r.end))
    if ((char)p[0] == a && (char)p[1] == b) return p + 2;
  return nullptr;
}

// whether a walk over the record's aux fields (as aux_z makes it) ends exactly at the record's end: tags appended to
// the record are then found by a later walk, otherwise they lie beyond a malformed field and are not
static inline bool aux_clean(const Rec &r) {
  const uint8_t *p = r.aux;
  while (p && p + 3 <= r.end) p = aux_value_end(p, r.end);
  return p == r.end;
}

// query bases (M I S = X) and reference bases (M D N = X) the CIGAR consumes; *bad_op: it holds an operation that BAM
// does not define (the lengths then leave it out)
static inline void cigar_lens(const Rec &r, uint64_t *qlen, uint64_t *rlen, bool *bad_op) {
  uint64_t q = 0, d = 0;
  bool bad = false;
  for (uint32_t i = 0; i < r.n_cigar; i++) {
    const uint32_t c = rd32(r.cigar + 4 * i), op = c & 0xF, len = c >> 4;
    if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) q += len;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) d += len;
    bad |= op > 9;
  }
  *qlen = q; *rlen = d; *bad_op = bad;
}

// ---- the window reader -------------------------------------------------------------------------------------------------
// the window of inflated bytes: grown without clearing it (std::vector::resize would zero-fill hundreds of megabytes on
// one thread before every inflate)
struct RawBuf {
  uint8_t *p = nullptr;
  size_t n = 0, cap = 0;
  ~RawBuf() { free(p); }
  uint8_t *data() { return p; }
  size_t size() const { return n; }
  uint8_t &operator[](size_t i) { return p[i]; }
  void resize(size_t m) {                                 // keeps the first n bytes (the carry)
    if (m > cap) {
      uint8_t *q = static_cast<uint8_t *>(big_malloc(m));
      if (!q) throw std::bad_alloc();
      if (n) memcpy(q, p, n);
      free(p);
      p = q; cap = m;
    }
    n = m;
  }
  void release() { free(p); p = nullptr; n = cap = 0; }
};

struct RecBuf {                                             // a window's records (not value-initialised: 80 bytes x millions)
  Rec *p = nullptr;
  size_t n = 0, cap = 0;
  ~RecBuf() { free(p); }
  size_t size() const { return n; }
  void clear() { n = 0; }
  Rec &operator[](size_t i) { return p[i]; }
  const Rec &operator[](size_t i) const { return p[i]; }
  const Rec *begin() const { return p; }
  const Rec *end() const { return p + n; }
  void resize_uninit(size_t m) {
    if (m > cap) {
      free(p);
      p = static_cast<Rec *>(big_malloc((m + m / 8 + 16) * sizeof(Rec)));
      if (!p) { cap = 0; n = 0; throw std::bad_alloc(); }
      cap = m + m / 8 + 16;
    }
    n = m;
  }
};

// The file as windows of inflated data (the reference streams records through HTSlib).  next() inflates a run of BGZF
// blocks behind what the last window left over, then indexes and parses the complete records; the caller takes records
// [0, r_end) and consume(r_end) carries the rest (a record cut by the window, or the records of a template whose mate is
// still to come) over to the next window.  keep_all() carries everything instead: the next window is this one and more.
class BamWindows {
 public:
  FileView file;                                             // the compressed file ...
  std::vector<Block> blocks;                                 // ... and its BGZF blocks
  std::vector<std::string> names;                            // the header's reference sequences ...
  std::vector<int64_t> lens;                                 // ... and their lengths (the genome check)
  RecBuf recs;                                               // the window's complete records
  double t_inflate = 0, t_parse = 0;                         // seconds spent so far (EPIHIP_BAM_TIMING)

  // window_kib 0: default_window bytes.  hdr_msg: the caller's words for a header that cannot be read.
  int open(const char *path, int32_t window_kib, size_t default_window, int nthreads, const char *hdr_msg);
  size_t inflated_size() const;
  // *final: the file's last block is in (what the window leaves over then is an error, or the caller's to take)
  int next(bool *final);
  // for the caller that needs more records at once than the window gave: fewer than .checkBam's 1024, or one template
  // that fills the window
  void keep_all() { carry_ = buf_.size(); }
  void consume(size_t r_end);
  const uint8_t *record(size_t i) { return buf_.data() + roff_[i]; }   // record i as the file has it, from its block_size
  const uint8_t *header() { return buf_.data(); }           // the header as the file has it: until the first consume()
  size_t header_size() const { return hdr_end_; }
  void release() { buf_.release(); }                         // after the last window

 private:
  struct Span { size_t p; uint32_t n; };                    // n records starting at byte p (a block, or a single record)
  int parse_header(bool *complete);
  size_t index_records(size_t kb, std::vector<Span> &spans);
  int parse_records(const std::vector<Span> &spans, size_t nrec);

  RawBuf buf_;                                               // [carry | the window's blocks]
  std::vector<size_t> roff_;                                 // offsets of the window's records in buf_
  size_t window_ = 0, carry_ = 0, bi_ = 0, hdr_end_ = 0, end_ = 0;   // end_: the byte after the last complete record
  int nthreads_ = 1;
  const char *hdr_msg_ = "";
  bool header_done_ = false;
};

}  // namespace bam
}  // namespace epi
