// Host-side producer: BAM file -> sorted, packed SoA templates in pinned host memory.
//
// Replaces the reference's
//   rcpp_check_bam            src/rcpp_check_bam.cpp:19-60   + .checkBam  R/internal.R:75-128
//   rcpp_read_bam_paired      src/rcpp_read_bam.cpp:19-192   (short-read XG/XM alignments)
//   rcpp_read_bam_single      src/rcpp_read_bam.cpp:199-343
//   rcpp_read_bam_mm_single   src/rcpp_read_bam.cpp:364-579  (long-read MM/ML alignments: pack_mm below)
//   .readBam (templid, sort)  R/internal.R:154-199
// without HTSlib: BGZF is a series of gzip members whose compressed size is in the
// BC extra field (SAM spec 4.1), so the blocks are located without inflating (the file is
// mmap-ed) and inflated in parallel by worker threads, window by window (a record or template
// that straddles a window seam is carried over); BAM records have a fixed layout (SAM spec 4.2)
// and are validated before use.  The packed byte per reference position is
// (nt16 << 4) | ctx_to_idx(XM) (src/epialleleR.h:28-35), filler 0xFB (N,'-').
// Output is what the GPU engine consumes: one contiguous byte stream in (rname,start)
// order + offsets + int32 columns, allocated with hipHostMalloc when a HIP device is
// usable (so it can be streamed to HBM with hipMemcpyAsync) and with malloc otherwise.
#include <hip/hip_runtime.h>
#include <zlib.h>
#include <dlfcn.h>
#include <stdio.h>
#include <limits.h>
#include <fcntl.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <deque>
#include <new>
#include <atomic>
#include <numeric>
#include <string>
#include <thread>
#include <chrono>
#include <vector>
#include "common.hpp"

using namespace epi;

namespace {

// Large host buffers (the inflated window, the packed bytes of a thread, the record index): 2 MiB-aligned and advised
// as huge pages -- a first touch then faults 2 MiB at a time instead of 4 KiB (hundreds of thousands of faults per file
// from 16 threads otherwise).  Released with free().
inline void *big_malloc(size_t bytes) {
  constexpr size_t HUGE = (size_t)2 << 20;
  if (bytes >= 4 * HUGE && !epi::options().no_hugepage) {
    const size_t r = (bytes + HUGE - 1) & ~(HUGE - 1);
    void *p = aligned_alloc(HUGE, r);
    if (p) { (void)madvise(p, r, MADV_HUGEPAGE); return p; }
  }
  return malloc(bytes);
}
template <class T> struct BigAlloc {
  using value_type = T;
  BigAlloc() = default;
  template <class U> BigAlloc(const BigAlloc<U> &) {}
  T *allocate(size_t n) { void *p = big_malloc(n * sizeof(T)); if (!p) throw std::bad_alloc(); return static_cast<T *>(p); }
  void deallocate(T *p, size_t) { free(p); }
  template <class U> bool operator==(const BigAlloc<U> &) const { return true; }
  template <class U> bool operator!=(const BigAlloc<U> &) const { return false; }
};

struct Block {
  size_t cpos, clen; size_t upos, ulen;                     // compressed payload / uncompressed placement
  // what the inflating thread found when it walked the block's bytes as a chain of BAM records starting at the block's
  // first byte: their number, and whether the chain ends exactly at the block's end.  (HTSlib never lets a record
  // straddle two blocks unless it is larger than one, so this is the true chain nearly always -- the index uses it
  // only where the true chain does arrive at the block's first byte.)
  uint32_t spec_n = 0;
  bool spec_ok = false;
};

inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint16_t rd16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }

// The compressed file, memory-mapped (read into a buffer where mmap is not possible): nothing of it is copied.
struct FileView {
  const uint8_t *p = nullptr;
  size_t n = 0;
  bool mapped = false;
  std::vector<uint8_t> own;
  ~FileView() { if (mapped && p) munmap(const_cast<uint8_t *>(p), n); }
};

int open_file(const char *path, FileView &v) {
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return fail(EPI_ERR_ARG, "Unable to open BAM file for reading");   // src/rcpp_read_bam.cpp:34
  struct stat st;
  if (fstat(fd, &st) != 0 || st.st_size < 0) { close(fd); return fail(EPI_ERR_ARG, "Unable to read BAM file"); }
  v.n = (size_t)st.st_size;
  if (v.n == 0) { close(fd); return EPI_OK; }
  void *m = mmap(nullptr, v.n, PROT_READ, MAP_PRIVATE, fd, 0);
  if (m != MAP_FAILED) { v.p = static_cast<const uint8_t *>(m); v.mapped = true; close(fd); return EPI_OK; }
  v.own.resize(v.n);
  size_t got = 0;
  while (got < v.n) {
    const ssize_t k = read(fd, v.own.data() + got, v.n - got);
    if (k <= 0) break;
    got += (size_t)k;
  }
  close(fd);
  if (got != v.n) return fail(EPI_ERR_ARG, "Unable to read BAM file");
  v.p = v.own.data();
  return EPI_OK;
}

// Locate the BGZF blocks (no inflation).
int bgzf_scan(const uint8_t *in, size_t n, std::vector<Block> &blocks) {
  size_t p = 0;
  while (p + 18 <= n) {
    const uint8_t *h = in + p;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return fail(EPI_ERR_ARG, "not a BGZF/BAM file");
    const unsigned xlen = rd16(h + 10);
    size_t q = p + 12;
    const size_t xend = p + 12 + xlen;
    int bsize = -1;
    while (q + 4 <= xend && xend <= n) {
      const unsigned slen = rd16(in + q + 2);
      if (in[q] == 'B' && in[q + 1] == 'C' && slen == 2 && q + 6 <= xend) bsize = rd16(in + q + 4);
      q += 4 + slen;
    }
    if (bsize < 0 || p + (size_t)bsize + 1 > n) return fail(EPI_ERR_ARG, "truncated BGZF block");
    const size_t blen = (size_t)bsize + 1;
    if (blen < (xend - p) + 8) return fail(EPI_ERR_ARG, "corrupt BGZF block");
    Block b;
    b.cpos = xend;
    b.clen = blen - (xend - p) - 8;
    b.ulen = rd32(in + p + blen - 4);
    b.upos = 0;
    if (b.ulen > 65536) return fail(EPI_ERR_ARG, "corrupt BGZF block");
    blocks.push_back(b);
    p += blen;
  }
  if (p != n) return fail(EPI_ERR_ARG, "truncated BGZF block");
  return EPI_OK;
}

// libdeflate (its shared library ships with the image; 2-3x zlib's inflate rate) is used when it can be loaded at run
// time -- no headers needed for its three-call ABI -- and zlib otherwise.  Both produce the same bytes or an error.
struct FastInflate {
  void *(*alloc)() = nullptr;
  int (*run)(void *, const void *, size_t, void *, size_t, size_t *) = nullptr;
  void (*release)(void *) = nullptr;
  FastInflate() {
    if (epi::options().no_libdeflate) return;
    void *h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
    alloc = reinterpret_cast<void *(*)()>(dlsym(h, "libdeflate_alloc_decompressor"));
    run = reinterpret_cast<int (*)(void *, const void *, size_t, void *, size_t, size_t *)>(dlsym(h, "libdeflate_deflate_decompress"));
    release = reinterpret_cast<void (*)(void *)>(dlsym(h, "libdeflate_free_decompressor"));
    if (!alloc || !run || !release) { alloc = nullptr; run = nullptr; release = nullptr; }
  }
  bool ok() const { return run != nullptr; }
};
const FastInflate &fast_inflate() { static const FastInflate f; return f; }

// Inflate blocks [b0, b1) to out + their upos, in parallel.
int bgzf_inflate_range(const uint8_t *in, std::vector<Block> &blocks, size_t b0, size_t b1, uint8_t *out, int nthreads) {
  std::atomic<size_t> next(b0);
  std::atomic<int> bad(0);
  auto walk = [&](Block &b) {                                // (the bytes are still in this core's cache)
    const uint8_t *q = out + b.upos;
    size_t p = 0;
    uint32_t n = 0;
    while (p + 4 <= b.ulen) {
      const size_t bs = rd32(q + p);
      if (p + 4 + bs > b.ulen) break;
      p += 4 + bs;
      n++;
    }
    b.spec_n = n;
    b.spec_ok = p == b.ulen;
  };
  auto work = [&]() {
    const FastInflate &fi = fast_inflate();
    if (fi.ok()) {
      void *d = fi.alloc();
      if (d) {
        for (;;) {
          const size_t i = next.fetch_add(1);
          if (i >= b1) break;
          Block &b = blocks[i];
          b.spec_n = 0; b.spec_ok = false;
          if (b.ulen == 0) continue;
          size_t got = 0;
          if (fi.run(d, in + b.cpos, b.clen, out + b.upos, b.ulen, &got) != 0 || got != b.ulen) bad = 1;
          else walk(b);
        }
        fi.release(d);
        return;
      }
    }
    z_stream zs;                                             // one stream per thread, reset per block (an init / end pair per
    memset(&zs, 0, sizeof(zs));                              // block allocates and frees its state and window every 64 KiB)
    if (inflateInit2(&zs, -15) != Z_OK) { bad = 1; return; }
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= b1) break;
      Block &b = blocks[i];
      b.spec_n = 0; b.spec_ok = false;
      if (b.ulen == 0) continue;
      if (inflateReset(&zs) != Z_OK) { bad = 1; continue; }
      zs.next_in = const_cast<Bytef *>(in + b.cpos);
      zs.avail_in = (uInt)b.clen;
      zs.next_out = out + b.upos;
      zs.avail_out = (uInt)b.ulen;
      const int rc = inflate(&zs, Z_FINISH);
      if (rc != Z_STREAM_END || zs.avail_out != 0) bad = 1;
      else walk(b);
    }
    inflateEnd(&zs);
  };
  int nt = nthreads > 0 ? nthreads : 1;
  if ((size_t)nt > b1 - b0) nt = b1 > b0 ? (int)(b1 - b0) : 1;
  std::vector<std::thread> th;
  for (int t = 1; t < nt; t++) th.emplace_back(work);
  work();
  for (auto &t : th) t.join();
  if (bad) return fail(EPI_ERR_ARG, "corrupt BGZF block");
  return EPI_OK;
}

inline double tnow() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the caller's nthreads -> threads of the host loops below (the inflate takes nthreads as given)
inline size_t thread_cap(int nthreads) { return nthreads > 1 ? (size_t)(nthreads > 16 ? 16 : nthreads) : 1; }

// [0, n) in K nearly equal ranges: the K + 1 cut points
inline std::vector<size_t> even_cuts(size_t n, size_t K) {
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
bool parse_record(const uint8_t *b, uint32_t bs, Rec *r) {
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
inline const uint8_t *aux_value_end(const uint8_t *p, const uint8_t *end) {
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
const char *aux_z(const Rec &r, char a, char b, bool *present) {
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

bool has_tag(const Rec &r, char a, char b) { bool pr; (void)aux_z(r, a, b, &pr); return pr; }

// bam_aux_get for B-typed (array) tags: element type, count and a pointer to the first element; false if absent.  Every
// array on the way, the tag's own included, must lie inside the record.
bool aux_b(const Rec &r, char a, char b, char *sub, uint32_t *count, const uint8_t **data) {
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
const uint8_t *aux_find(const Rec &r, char a, char b) {
  for (const uint8_t *p = r.aux; p && p + 3 <= r.end; p = aux_value_end(p, r.end))
    if ((char)p[0] == a && (char)p[1] == b) return p + 2;
  return nullptr;
}

// whether a walk over the record's aux fields (as aux_z makes it) ends exactly at the record's end: tags appended to
// the record are then found by a later walk, otherwise they lie beyond a malformed field and are not
bool aux_clean(const Rec &r) {
  const uint8_t *p = r.aux;
  while (p && p + 3 <= r.end) p = aux_value_end(p, r.end);
  return p == r.end;
}

// query bases (M I S = X) and reference bases (M D N = X) the CIGAR consumes; *bad_op: it holds an operation that BAM
// does not define (the lengths then leave it out)
inline void cigar_lens(const Rec &r, uint64_t *qlen, uint64_t *rlen, bool *bad_op) {
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
  int open(const char *path, int32_t window_kib, size_t default_window, int nthreads, const char *hdr_msg) {
    window_ = window_kib > 0 ? (size_t)window_kib * 1024 : default_window;
    nthreads_ = nthreads;
    hdr_msg_ = hdr_msg;
    EPI_TRY(open_file(path, file));
    return bgzf_scan(file.p, file.n, blocks);
  }
  size_t inflated_size() const {
    size_t total = 0;
    for (const Block &b : blocks) total += b.ulen;
    return total;
  }

  // *final: the file's last block is in (what the window leaves over then is an error, or the caller's to take)
  int next(bool *final) {
    for (;;) {
      double tw = tnow();
      const size_t b0 = bi_;                                 // first block inflated into this window
      size_t add = 0;
      while (bi_ < blocks.size() && (bi_ == b0 || add + blocks[bi_].ulen <= window_)) { blocks[bi_].upos = carry_ + add; add += blocks[bi_].ulen; bi_++; }
      *final = bi_ == blocks.size();
      buf_.resize(carry_ + add);
      EPI_TRY(bgzf_inflate_range(file.p, blocks, b0, bi_, buf_.data(), nthreads_));
      t_inflate += tnow() - tw;
      tw = tnow();
      if (!header_done_) {
        bool complete = false;
        EPI_TRY(parse_header(&complete));
        if (!complete) {
          if (*final) return fail(EPI_ERR_ARG, "%s", hdr_msg_);
          keep_all();                                        // the header is longer than a window: read on
          continue;
        }
        header_done_ = true;
      }
      std::vector<Span> spans;
      const size_t nrec = index_records(b0, spans);
      EPI_TRY(parse_records(spans, nrec));
      if (*final && end_ != buf_.size()) return fail(EPI_ERR_ARG, "truncated BAM record");
      t_parse += tnow() - tw;
      return EPI_OK;
    }
  }
  // for the caller that needs more records at once than the window gave: fewer than .checkBam's 1024, or one template
  // that fills the window
  void keep_all() { carry_ = buf_.size(); }
  void consume(size_t r_end) {
    const size_t keep_from = r_end < recs.size() ? roff_[r_end] : end_;
    carry_ = buf_.size() - keep_from;
    if (carry_) memmove(buf_.data(), buf_.data() + keep_from, carry_);
    hdr_end_ = 0;                                            // (the header is gone from the buffer)
    recs.clear();
  }
  const uint8_t *record(size_t i) { return buf_.data() + roff_[i]; }   // record i as the file has it, from its block_size
  const uint8_t *header() { return buf_.data(); }           // the header as the file has it: until the first consume()
  size_t header_size() const { return hdr_end_; }
  void release() { buf_.release(); }                         // after the last window

 private:
  struct Span { size_t p; uint32_t n; };                    // n records starting at byte p (a block, or a single record)

  // BAM header: magic, text, reference names and lengths.  *complete: all of it is in the buffer, up to hdr_end_.
  int parse_header(bool *complete) {
    *complete = false;
    if (buf_.size() < 12) return EPI_OK;
    if (memcmp(buf_.data(), "BAM\1", 4) != 0) return fail(EPI_ERR_ARG, "%s", hdr_msg_);
    size_t q = 8 + (size_t)rd32(buf_.data() + 4);
    if (q + 4 > buf_.size()) return EPI_OK;
    const uint32_t n_ref = rd32(buf_.data() + q);
    q += 4;
    names.clear(); lens.clear();
    for (uint32_t i = 0; i < n_ref; i++) {
      if (q + 4 > buf_.size()) return EPI_OK;
      const uint32_t l = rd32(buf_.data() + q);
      if (q + 4 + (size_t)l + 4 > buf_.size()) return EPI_OK;
      if (l == 0 || buf_[q + 4 + l - 1] != 0) return fail(EPI_ERR_ARG, "%s", hdr_msg_);
      names.emplace_back((const char *)buf_.data() + q + 4);
      lens.push_back((int64_t)rd32(buf_.data() + q + 4 + l));
      q += 4 + (size_t)l + 4;
    }
    hdr_end_ = q;
    *complete = true;
    return EPI_OK;
  }

  // Index of the complete records of the window.  The chain of block sizes is followed from the first record; wherever
  // it arrives exactly at the first byte of a BGZF block whose own walk (done by the thread that inflated it) ended
  // exactly at the block's end, the block's records are taken as a whole -- they are enumerated and parsed by all
  // threads in parse_records -- so the serial part is one step per block, not per record.
  size_t index_records(size_t kb, std::vector<Span> &spans) {
    size_t p = hdr_end_, nrec = 0;
    for (;;) {
      while (kb < bi_ && blocks[kb].upos < p) kb++;
      if (kb < bi_ && blocks[kb].upos == p && blocks[kb].spec_ok && blocks[kb].spec_n > 0) {
        spans.push_back({p, blocks[kb].spec_n});
        nrec += blocks[kb].spec_n;
        p += blocks[kb].ulen;
        continue;
      }
      if (p + 4 > buf_.size()) break;
      const uint32_t bs = rd32(buf_.data() + p);
      if (p + 4 + (size_t)bs > buf_.size()) break;           // cut by the window (or by the end of the file)
      spans.push_back({p, 1u});
      nrec++;
      p += 4 + (size_t)bs;
    }
    end_ = p;
    return nrec;
  }

  int parse_records(const std::vector<Span> &spans, size_t nrec) {
    recs.resize_uninit(nrec);
    roff_.resize(nrec);
    std::vector<size_t> base(spans.size() + 1, 0);
    for (size_t i = 0; i < spans.size(); i++) base[i + 1] = base[i] + spans[i].n;
    std::atomic<size_t> next(0);
    const size_t K = nrec < 4096 ? 1 : thread_cap(nthreads_);
    // (a part is a thread here, not a range: each takes a few spans at a time until none is left)
    return fan_out(even_cuts(K, K), "epi_preprocess_bam", "reading records", [&](size_t, size_t, size_t) -> int {
      for (;;) {
        const size_t i0 = next.fetch_add(16);
        if (i0 >= spans.size()) return EPI_OK;
        const size_t i1 = i0 + 16 < spans.size() ? i0 + 16 : spans.size();
        for (size_t i = i0; i < i1; i++) {
          size_t q = spans[i].p;
          for (size_t j = base[i]; j < base[i + 1]; j++) {
            const uint8_t *rp = buf_.data() + q;
            const uint32_t bs = rd32(rp);
            roff_[j] = q;
            if (!parse_record(rp + 4, bs, &recs[j])) return fail(EPI_ERR_ARG, "corrupt BAM record");
            q += 4 + (size_t)bs;
          }
        }
      }
    });
  }

  RawBuf buf_;                                               // [carry | the window's blocks]
  std::vector<size_t> roff_;                                 // offsets of the window's records in buf_
  size_t window_ = 0, carry_ = 0, bi_ = 0, hdr_end_ = 0, end_ = 0;   // end_: the byte after the last complete record
  int nthreads_ = 1;
  const char *hdr_msg_ = "";
  bool header_done_ = false;
};

inline uint8_t ctx_idx(char c) { return (uint8_t)ctx_to_idx((unsigned char)c); }
inline uint8_t seqi_shifted(const uint8_t *s, uint32_t i) { return (uint8_t)((s[i >> 1] << ((i & 1) << 2)) & 0xF0); }   // epialleleR.h:32

// ---- long-read (MM/ML) records -------------------------------------------------------------------------------
// The reference leaves the MM/ML tags to HTSlib (bam_parse_basemod / bam_next_basemod; Rhtslib, version not pinned in
// DESCRIPTION).  HTSlib is not part of the reference tree, so this restates the published rules of the SAM tags
// specification (SAMtags.pdf section 1.7 "Base modifications"):
//   MM:Z:  ([ACGTUN][-+]([a-z]+|[0-9]+)[.?]?(,[0-9]+)*;)*   one entry per (canonical base, strand, modification codes);
//          each number = how many bases of that canonical type to skip before the next modified one, counted along
//          the read AS SEQUENCED: for a reverse-strand alignment from the end of SEQ, on the complemented base;
//          base N counts every base; several one-letter codes in one entry share the positions.
//   ML:B:C one probability (0..255) per listed position and code, in MM order, codes of an entry interleaved per
//          position.  Without ML the probability is unknown (-1, as HTSlib reports it).
// A ChEBI number n is carried as code -n (HTSlib's convention, which rcpp_read_bam.cpp:474 relies on for 27551).
struct ModHit { int32_t pos; int32_t code; int32_t strand; int32_t qual; };

inline int nt16_of(char c) {
  switch (c) { case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': case 'U': return 8; case 'N': return 15; default: return -1; }
}
inline int nt16_complement(int c) { return c == 1 ? 8 : c == 8 ? 1 : c == 2 ? 4 : c == 4 ? 2 : c; }
inline int seqi(const uint8_t *s, uint32_t i) { return (s[i >> 1] >> ((~i & 1) << 2)) & 0xF; }

void parse_basemods(const Rec &r, const char *mm, bool has_ml, const uint8_t *ml, uint32_t n_ml, std::vector<ModHit> &hits) {
  hits.clear();
  const bool rev = (r.flag & 16) != 0;
  const int32_t L = r.l_seq;
  uint32_t ml_idx = 0;
  const char *p = mm;
  while (*p) {
    const int base = nt16_of(*p);
    if (base < 0) return;                                        // malformed: HTSlib gives up on the tag
    p++;
    if (*p != '+' && *p != '-') return;
    const int32_t strand = *p == '-' ? 1 : 0;
    p++;
    int32_t codes[16];
    int ncodes = 0;
    if (*p >= '0' && *p <= '9') {                                // one ChEBI number
      long v = 0;
      while (*p >= '0' && *p <= '9') { v = v * 10 + (*p - '0'); p++; }
      codes[ncodes++] = (int32_t)-v;
    } else {
      while (*p >= 'a' && *p <= 'z') { if (ncodes < 16) codes[ncodes++] = (int32_t)*p; p++; }
    }
    if (ncodes == 0) return;
    if (*p == '.' || *p == '?') p++;                             // implicit / explicit mode: only listed bases matter here
    const int target = rev ? nt16_complement(base) : base;
    int32_t i = rev ? L - 1 : 0;                                 // next base of SEQ to look at, in sequencing order
    const int32_t step = rev ? -1 : 1;
    while (*p == ',') {
      p++;
      long skip = 0;
      if (!(*p >= '0' && *p <= '9')) return;
      while (*p >= '0' && *p <= '9') { skip = skip * 10 + (*p - '0'); p++; }
      // advance to the (skip+1)-th base of the canonical type
      int32_t found = -1;
      while (i >= 0 && i < L) {
        const bool match = target == 15 || seqi(r.seq, (uint32_t)i) == target;
        const int32_t at = i;
        i += step;
        if (match) { if (skip == 0) { found = at; break; } skip--; }
      }
      if (found < 0) return;                                     // the tag points beyond the sequence
      for (int k = 0; k < ncodes; k++) {
        ModHit h;
        h.pos = found; h.code = codes[k]; h.strand = strand;
        h.qual = has_ml ? (ml_idx < n_ml ? (int32_t)ml[ml_idx] : -1) : -1;
        ml_idx++;
        hits.push_back(h);
      }
    }
    if (*p != ';') return;
    p++;
  }
}

// cytosine context of query base i from the base and its two neighbours, keyed like the reference's 512-entry tables
// (src/epialleleR.h:43-116) by the low three bits of the IUPAC letters: A=1 C=3 T=4 N=6 G=7, anything else gives '.'
inline bool tri_ok(int c) { return c == 1 || c == 3 || c == 4 || c == 6 || c == 7; }
inline char ctx_forward(int b0, int b1, int b2) {                // C at i: CG -> z, CHG -> x, CHH -> h
  if (b0 != 3 || !tri_ok(b1) || !tri_ok(b2)) return '.';
  return b1 == 7 ? 'z' : b2 == 7 ? 'x' : 'h';
}
inline char ctx_reverse(int b0, int b1, int b2) {                // G at i with (i-2, i-1, i): CG -> z, CHG -> x, CHH -> h
  if (b2 != 7 || !tri_ok(b0) || !tri_ok(b1)) return '.';
  return b1 == 3 ? 'z' : b0 == 3 ? 'x' : 'h';
}

struct Packed {
  std::vector<int32_t> rname, strand, start;
  std::vector<int64_t> off;          // template t owns bytes [off[t], off[t+1])
  std::vector<uint8_t, BigAlloc<uint8_t>> bytes;
  // one template: 1-based rname and start, and row[0, width) less both trims (src/rcpp_read_bam.cpp:61-69, 303-306,
  // 537-541)
  void push_row(int32_t tid, int32_t strand_, int32_t pos, const uint8_t *row, int width, int trim5, int trim3) {
    rname.push_back(tid + 1);
    strand.push_back(strand_);
    start.push_back(pos + trim5 + 1);
    const int keep = width - (trim5 + trim3);
    if (keep > 0) bytes.insert(bytes.end(), row + trim5, row + trim5 + keep);
    off.push_back((int64_t)bytes.size());
  }
};

// (nt16 << 4) | ctx_idx(XM) of every query base of a record (src/epialleleR.h:28,32): two bases per byte of SEQ
inline void pack_query(const Rec &r, const char *xm, uint8_t *__restrict__ o) {
  const size_t n = (size_t)r.l_seq;
  const uint8_t *__restrict__ s = r.seq;
  const unsigned char *__restrict__ x = reinterpret_cast<const unsigned char *>(xm);
  for (size_t i = 0; i + 1 < n; i += 2) {
    const uint8_t b = s[i >> 1];
    o[i] = (uint8_t)((b & 0xF0) | (((x[i] + 2u) >> 2) & 15u));
    o[i + 1] = (uint8_t)(((b << 4) & 0xF0) | (((x[i + 1] + 2u) >> 2) & 15u));
  }
  if (n & 1) o[n - 1] = (uint8_t)((s[(n - 1) >> 1] & 0xF0) | (((x[n - 1] + 2u) >> 2) & 15u));
}
inline void packed_bytes(const Rec &r, const char *xm, std::vector<uint8_t> &pb) {
  pb.resize((size_t)r.l_seq + 2);
  pack_query(r, xm, pb.data());
}

// walk the CIGAR of one record into the template buffers; returns the reference position after the last op
template <class F>
int apply_cigar(const Rec &r, uint32_t dest0, F &&on_match, uint32_t *dest_end) {
  uint32_t qpos = 0, dpos = dest0;
  for (uint32_t i = 0; i < r.n_cigar; i++) {
    const uint32_t c = rd32(r.cigar + 4 * i), op = c & 0xF, len = c >> 4;
    switch (op) {
      case 0: case 7: case 8: on_match(qpos, dpos, len); qpos += len; dpos += len; break;    // M = X
      case 1: case 4: qpos += len; break;                                                     // I S
      case 2: case 3: dpos += len; break;                                                     // D N
      case 5: case 6: case 9: break;                                                          // H P B
      default: return fail(EPI_ERR_ARG, "Unknown CIGAR operation for BAM entry %s", r.qname);
    }
  }
  *dest_end = dpos;
  return EPI_OK;
}

// QNAME -> template id (mates = "anywhere"), ids given in the order the keys are first added.  Open addressing over a
// power-of-two table with the exact string compare; the keys are kept back to back (NUL-terminated), which also names
// the template in messages after its records' window is gone.
class QnameMap {
 public:
  static uint64_t hash(const char *q) {                      // FNV-1a, finalised
    uint64_t h = 0xCBF29CE484222325ull;
    for (; *q; q++) h = (h ^ (uint8_t)*q) * 0x100000001B3ull;
    return mix64(h);
  }
  uint32_t find_or_add(const char *q, uint64_t h) {
    if (2 * (hash_.size() + 1) > slot_.size()) grow();
    const size_t mask = slot_.size() - 1;
    size_t i = (size_t)h & mask;
    for (; slot_[i]; i = (i + 1) & mask) {
      const uint32_t g = slot_[i] - 1;
      if (hash_[g] == h && strcmp(name(g), q) == 0) return g;
    }
    const uint32_t g = (uint32_t)hash_.size();
    slot_[i] = g + 1;
    hash_.push_back(h);
    off_.push_back(names_.size());
    names_.insert(names_.end(), q, q + strlen(q) + 1);
    return g;
  }
  const char *name(uint32_t g) const { return names_.data() + off_[g]; }
  size_t size() const { return hash_.size(); }

 private:
  void grow() {
    slot_.assign(slot_.empty() ? 4096 : 2 * slot_.size(), 0u);
    const size_t mask = slot_.size() - 1;
    for (uint32_t g = 0; g < (uint32_t)hash_.size(); g++) {
      size_t i = (size_t)hash_[g] & mask;
      while (slot_[i]) i = (i + 1) & mask;
      slot_[i] = g + 1;
    }
  }
  std::vector<uint32_t> slot_;     // id + 1, 0: empty
  std::vector<uint64_t> hash_;     // per id
  std::vector<size_t> off_;        // per id: its key in names_
  std::vector<char> names_;
};

// ---- callMethylation's call set (rcpp_call_methylation_genome, src/rcpp_call_methylation.cpp:27-177, with
// .callMethylation's tag choice, R/internal.R:405-432): which records are called and what the GPU needs for them.
// Shared by callMethylation (BAM out, call_impl below) and preprocessBam with a genome (preprocess_impl), so that the
// second sees exactly the records, strand letters and errors the first would have produced. ----------------------
enum StrandTag { TAG_XG = 0, TAG_YD = 1, TAG_ZS = 2 };

// .callMethylation (R/internal.R:412-423): the strand tag from the first 1024 records; force_tag ("XG" / "YD" / "ZS")
// skips the look (rcpp_call_methylation_genome's own contract)
int call_choose_tag(const Rec *recs, size_t nrec, const char *force_tag, StrandTag *tag) {
  bool tXG = false, tYD = false, tZS = false;
  for (size_t i = 0; i < nrec && i < 1024; i++) {
    tXG |= aux_find(recs[i], 'X', 'G') != nullptr;
    tYD |= aux_find(recs[i], 'Y', 'D') != nullptr;
    tZS |= aux_find(recs[i], 'Z', 'S') != nullptr;
  }
  if (force_tag) *tag = strcmp(force_tag, "XG") == 0 ? TAG_XG : strcmp(force_tag, "YD") == 0 ? TAG_YD : TAG_ZS;
  else if (nrec == 0) return fail(EPI_ERR_ARG, "Empty file provided! Exiting");
  else if (tXG) *tag = TAG_XG;
  else if (tYD) *tag = TAG_YD;
  else if (tZS) *tag = TAG_ZS;
  else return fail(EPI_ERR_ARG, "Unable to call methylation: neither of XG/YD/ZS tags is present (genome strand unknown).\nExiting");
  return EPI_OK;
}

// the header's reference sequences must be the genome's, by name and length (src/rcpp_call_methylation.cpp:41-72)
int call_check_genome(epi_genome *g, const std::vector<std::string> &names, const std::vector<int64_t> &lens) {
  const int32_t ng = epi_genome_count(g);
  for (size_t i = 0; i < names.size(); i++)
    if ((int32_t)i >= ng || epi_genome_length(g, (int32_t)i) != lens[i] || names[i] != epi_genome_name(g, (int32_t)i))
      return fail(EPI_ERR_ARG, "BAM reference sequence doesn't match the provided genome sequence");
  return EPI_OK;
}

struct CallSet {                      // the records of one window to call
  std::vector<uint8_t> call;          // per record: 1 = call it
  std::vector<uint8_t> s_meth, s_conv;
  std::vector<int64_t> call_idx;      // per called record of the packed range: its index among the called ones
  std::vector<CallRec> crec;
  std::vector<uint32_t> cigar;
  std::vector<uint8_t> seq;
  std::vector<uint8_t> xm;            // the GPU's output: l_seq bytes per called record, at its xm_off
  int64_t ncig = 0, nseq = 0, nxm = 0;
};

// Which of recs[0, n) are called (mapped, carrying the strand tag, no XM: :84-89), their strand letters (the tag's first
// two characters, or the strand YD / ZS names: :92-97), and the checks that keep every access in bounds (DESIGN.md
// section 2: the reference reads out of bounds here).  A called record grows by the XG tag (YD / ZS input) and XM.
int call_select(const Rec *recs, size_t n, StrandTag tag, const std::vector<std::string> &names,
                const std::vector<int64_t> &lens, size_t K, const char *who, CallSet &S) {
  const char t0 = tag == TAG_XG ? 'X' : tag == TAG_YD ? 'Y' : 'Z', t1 = tag == TAG_XG ? 'G' : tag == TAG_YD ? 'D' : 'S';
  S.call.resize(n); S.s_meth.resize(n); S.s_conv.resize(n);
  return parallel_ranges(K, n, who, [&](size_t lo, size_t hi) -> int {
    for (size_t i = lo; i < hi; i++) {
      const Rec &r = recs[i];
      S.call[i] = 0;
      const uint8_t *st = aux_find(r, t0, t1);
      if ((r.flag & 4) || !st || aux_find(r, 'X', 'M')) continue;          // written unchanged
      // the strand tag's first two characters (bam_aux_get's pointer [1] and [2])
      const uint8_t c1 = st + 1 < r.end ? st[1] : 0, c2 = st + 2 < r.end ? st[2] : 0;
      if (tag == TAG_XG) { S.s_meth[i] = c1; S.s_conv[i] = c2; }
      else {
        const bool ga = tag == TAG_YD ? c1 == 'r' : c1 == '-';
        S.s_meth[i] = ga ? 'G' : 'C'; S.s_conv[i] = ga ? 'A' : 'T';
      }
      if (r.tid < 0 || (size_t)r.tid >= names.size()) return fail(EPI_ERR_ARG, "corrupt BAM record %s: reference id out of range", r.qname);
      if (r.pos < 0) return fail(EPI_ERR_ARG, "corrupt BAM record %s: position out of range", r.qname);
      uint64_t qlen, rlen;
      bool bad_op;
      cigar_lens(r, &qlen, &rlen, &bad_op);
      if (bad_op) return fail(EPI_ERR_ARG, "Unknown CIGAR operation for BAM entry %s", r.qname);
      if (qlen != (uint64_t)r.l_seq) return fail(EPI_ERR_ARG, "corrupt BAM record %s: CIGAR does not match the sequence length", r.qname);
      if ((uint64_t)r.pos + rlen > (uint64_t)lens[(size_t)r.tid])
        return fail(EPI_ERR_ARG, "corrupt BAM record %s: alignment runs past the end of reference sequence %s", r.qname, names[(size_t)r.tid].c_str());
      const uint64_t bs = (uint64_t)(r.end - (const uint8_t *)r.qname) + 32;   // block_size (the name follows 32 fixed bytes)
      if (bs + (tag == TAG_XG ? 0 : 6) + 4 + (uint64_t)r.l_seq > 0x7FFFFFFFull)
        return fail(EPI_ERR_ARG, "corrupt BAM record %s: record too large", r.qname);
      S.call[i] = 1;
    }
    return EPI_OK;
  });
}

// the CallRec, CIGAR and SEQ inputs of the called records among recs[0, n) (n: at most call_select's range)
int call_pack_inputs(const Rec *recs, size_t n, size_t K, const char *who, CallSet &S) {
  S.call_idx.resize(n);
  S.crec.clear();
  int64_t ncig = 0, nseq = 0, nxm = 0;
  for (size_t i = 0; i < n; i++) {
    if (!S.call[i]) continue;
    const Rec &r = recs[i];
    CallRec c;
    memset(&c, 0, sizeof(c));
    c.cig_off = ncig; c.seq_off = nseq; c.xm_off = nxm;
    c.tid = r.tid; c.pos = r.pos; c.l_seq = r.l_seq; c.n_cig = (int32_t)r.n_cigar;
    c.s_meth = S.s_meth[i]; c.s_conv = S.s_conv[i];
    S.call_idx[i] = (int64_t)S.crec.size();
    S.crec.push_back(c);
    ncig += r.n_cigar; nseq += ((int64_t)r.l_seq + 1) / 2; nxm += r.l_seq;
  }
  S.ncig = ncig; S.nseq = nseq; S.nxm = nxm;
  S.cigar.resize((size_t)ncig); S.seq.resize((size_t)nseq); S.xm.resize((size_t)nxm);
  return parallel_ranges(K, n, who, [&](size_t lo, size_t hi) -> int {
    for (size_t i = lo; i < hi; i++) {
      if (!S.call[i]) continue;
      const Rec &r = recs[i];
      const CallRec &c = S.crec[(size_t)S.call_idx[i]];
      if (r.n_cigar) memcpy(S.cigar.data() + c.cig_off, r.cigar, 4 * (size_t)r.n_cigar);
      if (r.l_seq) memcpy(S.seq.data() + c.seq_off, r.seq, ((size_t)r.l_seq + 1) / 2);
    }
    return EPI_OK;
  });
}

// ---- .readBam: skip flags (R/internal.R:173-177) and the packers ----
struct PackCtx {                      // what the packers read of the call's options and of the file; never written by them
  uint16_t skip_flags;
  int32_t min_mapq, min_baseq, min_prob, highest_prob, trim5, trim3;
  size_t n_ref;                       // the header's reference sequences
  const CallSet *calls;               // with a genome: the window's records called on the way in, else NULL
};

// XG's first letter and the XM bytes of record ri, as the packers see them: from its own tags, or -- a record called on
// the way in (genome) -- as callMethylation would have written it: its own XG, else the appended one (s_meth), and the
// appended XM, here the packed bytes the GPU made (*pcall).  false: not usable (no XG / XM string).
bool xg_xm(const PackCtx &c, size_t ri, const Rec &r, char *s, const char **xm, const uint8_t **pcall) {
  bool pg, pm;
  const char *xg = aux_z(r, 'X', 'G', &pg);
  *xm = nullptr; *pcall = nullptr;
  if (c.calls && c.calls->call[ri]) {
    if (!aux_clean(r) || (pg && !xg)) return false;         // (the appended tags cannot be reached / XG is not a string)
    *s = pg ? xg[0] : (char)c.calls->s_meth[ri];
    *pcall = c.calls->xm.data() + c.calls->crec[(size_t)c.calls->call_idx[ri]].xm_off;
    return true;
  }
  *xm = aux_z(r, 'X', 'M', &pm);
  if (!pg || !pm || !xg || !*xm) return false;
  *s = xg[0];
  return true;
}

// a record that enters a template must be self-consistent: the CIGAR consumes exactly the stored bases, XM covers
// them, the reference id exists (HTSlib rejects such records while reading; without the checks they index past
// the record).  *width: the reference bases the CIGAR spans (bam_cigar2rlen).
int use_record(const PackCtx &c, const Rec &r, const char *xm, uint32_t *width) {
  if (r.tid < 0 || (size_t)r.tid >= c.n_ref) return fail(EPI_ERR_ARG, "corrupt BAM record %s: reference id out of range", r.qname);
  uint64_t qlen, rlen;
  bool bad_op;                                              // (left to apply_cigar, which names it after these checks)
  cigar_lens(r, &qlen, &rlen, &bad_op);
  if (qlen != (uint64_t)r.l_seq) return fail(EPI_ERR_ARG, "corrupt BAM record %s: CIGAR does not match the sequence length", r.qname);
  if (xm && strlen(xm) < (size_t)r.l_seq) return fail(EPI_ERR_ARG, "corrupt BAM record %s: XM tag shorter than the sequence", r.qname);
  *width = (uint32_t)rlen;
  return EPI_OK;
}

// Each packer turns records [r_lo, r_hi) into templates appended to P; ranges are packed by several threads and
// concatenated in order (a paired-end range never starts inside a template).
int pack_mm(const PackCtx &c, const Rec *recs, size_t r_lo, size_t r_hi, Packed &P) {
  // ---- rcpp_read_bam_mm_single (src/rcpp_read_bam.cpp:364-579) ----
  static const char nt16_str[] = "=ACMGRSVTWYHKDBN";
  std::vector<char> seq, xm[2];
  std::vector<uint8_t> rs[2];
  std::vector<ModHit> hits;
  for (size_t ri = r_lo; ri < r_hi; ri++) {
    const Rec &r = recs[ri];
    if ((r.flag & c.skip_flags) || (int)r.mapq < c.min_mapq) continue;                        // :423-424
    uint32_t width;                                                                           // bam_cigar2rlen, :437
    EPI_TRY(use_record(c, r, nullptr, &width));
    const int record_strand = (r.flag & 16) ? 1 : 0;                                          // :426
    const int32_t qw = r.l_seq < 0 ? -r.l_seq : r.l_seq;                                      // :436
    rs[0].assign(width, 0xFB); rs[1].assign(width, 0xFB);                                     // :453-454
    seq.assign((size_t)qw + 4, 'N');                                                          // :457-461 NN + SEQ + NN
    for (int32_t i = 0; i < qw; i++) seq[(size_t)i + 2] = nt16_str[seqi(r.seq, (uint32_t)i)];
    xm[0].resize((size_t)qw); xm[1].resize((size_t)qw);
    for (int32_t i = 0; i < qw; i++) {                                                        // :464-467
      xm[0][(size_t)i] = ctx_forward(seq[(size_t)i + 2] & 7, seq[(size_t)i + 3] & 7, seq[(size_t)i + 4] & 7);
      xm[1][(size_t)i] = ctx_reverse(seq[(size_t)i] & 7, seq[(size_t)i + 1] & 7, seq[(size_t)i + 2] & 7);
    }
    bool strand_has_mods[2] = {false, false};
    bool pmm = false;
    const char *mm = aux_z(r, 'M', 'M', &pmm);
    if (!mm) mm = aux_z(r, 'M', 'm', &pmm);
    if (mm) {
      char sub = 0; uint32_t n_ml = 0; const uint8_t *ml = nullptr;
      bool has_ml = aux_b(r, 'M', 'L', &sub, &n_ml, &ml) || aux_b(r, 'M', 'l', &sub, &n_ml, &ml);
      if (has_ml && sub != 'C' && sub != 'c') has_ml = false;
      parse_basemods(r, mm, has_ml, ml, n_ml, hits);
      std::stable_sort(hits.begin(), hits.end(), [](const ModHit &x, const ModHit &y) { return x.pos < y.pos; });
      for (size_t a0 = 0; a0 < hits.size();) {                                                // one query position at a time, :469
        size_t a1 = a0;
        int ismeth[2] = {0, 0}, meth_prob[2] = {-2, -2}, max_other[2] = {-2, -2};             // :470-472
        for (; a1 < hits.size() && hits[a1].pos == hits[a0].pos; a1++) {
          const ModHit &h = hits[a1];
          if (h.code == 'm' || h.code == -27551) { ismeth[h.strand] = 1; meth_prob[h.strand] = h.qual; }   // :474-476
          else if (max_other[h.strand] < h.qual) max_other[h.strand] = h.qual;                             // :477-479
        }
        const int32_t mod_pos = hits[a0].pos;
        for (int sidx = 0; sidx < 2; sidx++) {                                                // :481-490
          const int cs = record_strand > sidx ? record_strand - sidx : sidx - record_strand;
          if (ismeth[sidx] && meth_prob[sidx] >= c.min_prob && (!c.highest_prob || meth_prob[sidx] > max_other[sidx]) &&
              xm[cs][(size_t)mod_pos] > 'A') {
            xm[cs][(size_t)mod_pos] &= (char)0xDF;
            strand_has_mods[cs] = true;
          }
        }
        a0 = a1;
      }
    }
    uint32_t dest_end = 0;
    EPI_TRY(apply_cigar(r, 0, [&](uint32_t qpos, uint32_t dpos, uint32_t len) {              // :494-531
      for (uint32_t j = 0; j < len; j++)
        if ((int)r.qual[qpos + j] >= c.min_baseq) {
          const uint8_t hi = seqi_shifted(r.seq, qpos + j);
          rs[0][dpos + j] = (uint8_t)(hi | ctx_idx(xm[0][qpos + j]));
          rs[1][dpos + j] = (uint8_t)(hi | ctx_idx(xm[1][qpos + j]));
        }
    }, &dest_end));
    strand_has_mods[record_strand] = true;                                                    // :534
    for (int sidx = 0; sidx < 2; sidx++)
      if (strand_has_mods[sidx]) P.push_row(r.tid, sidx + 1, r.pos, rs[sidx].data(), (int)dest_end, c.trim5, c.trim3);   // :537-541
  }
  return EPI_OK;
}

int pack_pe(const PackCtx &c, const Rec *recs, size_t r_lo, size_t r_hi, Packed &P) {
  const uint16_t skip_flags_pe = c.skip_flags | 8;
  const uint8_t q0 = (uint8_t)(c.min_baseq - (c.min_baseq > 0 ? 1 : 0));   // src/rcpp_read_bam.cpp:30,57
  std::vector<uint8_t> tq(8192, q0), ts(8192, 0xFB), pb;
  const char *tname = nullptr;
  int t_rname = 0, t_start = 0, t_strand = 0, t_width = 0;
  auto grow = [&](size_t w) { if (w > tq.size()) { tq.resize(w, q0); ts.resize(w, 0xFB); } };
  auto push_template = [&]() {                                                   // :61-69
    P.push_row(t_rname, t_strand, t_start, ts.data(), t_width, c.trim5, c.trim3);
    std::fill(tq.begin(), tq.begin() + t_width, q0);
    std::fill(ts.begin(), ts.begin() + t_width, (uint8_t)0xFB);
  };
  for (size_t ri = r_lo; ri < r_hi; ri++) {
    const Rec &r = recs[ri];
    if ((r.flag & skip_flags_pe) || !(r.flag & 0x2) || (int)r.mapq < c.min_mapq) continue;   // :76-78
    char xg0;
    const char *xm;
    const uint8_t *pcall;
    if (!xg_xm(c, ri, r, &xg0, &xm, &pcall)) continue;                                           // :80-82
    uint32_t width;
    EPI_TRY(use_record(c, r, xm, &width));
    if (!tname || strcmp(tname, r.qname) != 0) {                                              // :85
      if (t_strand != 0) push_template();
      tname = r.qname;
      t_rname = r.tid;
      t_start = r.pos < r.mpos ? r.pos : r.mpos;                                              // :92-93
      if (r.isize == INT32_MIN) return fail(EPI_ERR_ARG, "corrupt BAM record %s: template length", r.qname);
      t_width = r.isize < 0 ? -r.isize : r.isize;                                             // :94
      t_strand = 2 - (xg0 == 'C' ? 1 : 0);                                                    // :95
      grow((size_t)t_width);
    }
    uint32_t dest_end = 0;
    if (r.pos < t_start) return fail(EPI_ERR_ARG, "corrupt BAM record %s: starts before its template", r.qname);
    const uint32_t dest0 = (uint32_t)(r.pos - t_start);                                       // :118
    if (!pcall) packed_bytes(r, xm, pb);                                                      // (nt16 << 4) | ctx_idx per query base
    const uint8_t *pbase = pcall ? pcall : pb.data();
    EPI_TRY(apply_cigar(r, dest0, [&](uint32_t qpos, uint32_t dpos, uint32_t len) {
      grow((size_t)dpos + len);
      const uint8_t *__restrict__ ql = r.qual + qpos, *__restrict__ pq = pbase + qpos;
      uint8_t *__restrict__ tqd = tq.data() + dpos, *__restrict__ tsd = ts.data() + dpos;
      for (uint32_t j = 0; j < len; j++) {                                                    // :127 strictly higher quality wins
        const bool w = ql[j] > tqd[j];                                                        // (selects, not branches: the loop vectorises)
        tqd[j] = w ? ql[j] : tqd[j];
        tsd[j] = w ? pq[j] : tsd[j];
      }
    }, &dest_end));
    if (dest_end > 0x7FFFFFFFu) return fail(EPI_ERR_ARG, "corrupt BAM record %s: template too wide", r.qname);
    if (t_width < (int)dest_end) t_width = (int)dest_end;                                     // :151
    grow((size_t)t_width);                                                                    // (a CIGAR ending in D / N)
  }
  if (t_strand != 0) push_template();                                                         // :155 (preprocess_impl has the "none")
  return EPI_OK;
}

int pack_se(const PackCtx &c, const Rec *recs, size_t r_lo, size_t r_hi, Packed &P) {
  const int min_baseq = c.min_baseq;
  std::vector<uint8_t> buf, pb;
  for (size_t ri = r_lo; ri < r_hi; ri++) {
    const Rec &r = recs[ri];
    if ((r.flag & c.skip_flags) || (int)r.mapq < c.min_mapq) continue;                        // :240-241
    char xg0;
    const char *xm;
    const uint8_t *pcall;
    if (!xg_xm(c, ri, r, &xg0, &xm, &pcall)) continue;
    uint32_t width;                                                                           // bam_cigar2rlen, :255
    EPI_TRY(use_record(c, r, xm, &width));
    buf.assign(width, 0xFB);                                                                  // :265
    uint32_t dest_end = 0;
    if (!pcall) packed_bytes(r, xm, pb);
    const uint8_t *pbase = pcall ? pcall : pb.data();
    EPI_TRY(apply_cigar(r, 0, [&](uint32_t qpos, uint32_t dpos, uint32_t len) {
      const uint8_t *__restrict__ ql = r.qual + qpos, *__restrict__ pq = pbase + qpos;
      uint8_t *__restrict__ bd = buf.data() + dpos;
      for (uint32_t j = 0; j < len; j++) bd[j] = (int)ql[j] >= min_baseq ? pq[j] : bd[j];   // :278
    }, &dest_end));
    P.push_row(r.tid, xg0 == 'C' ? 1 : 2, r.pos, buf.data(), (int)dest_end, c.trim5, c.trim3);   // :303-306
  }
  return EPI_OK;
}

// The output bytes go to page-locked memory (the upload DMAs straight from it).  Pinning ~100 MB takes tens of
// milliseconds, so it starts when the file is opened, next to the inflate / pack work, sized by an estimate (a base is at
// least 2.5 bytes of record: half a byte of SEQ, QUAL, XM); a template set that turns out larger is allocated at the end
// instead.
struct PinAhead {
  std::thread th;
  void *p = nullptr;
  size_t cap = 0;
  bool ok = false;
  ~PinAhead() { release(); }
  void wait() { if (th.joinable()) th.join(); }
  void release() {
    wait();
#ifndef EPI_HOST_ONLY
    if (ok && p) (void)hipHostFree(p);
#endif
    p = nullptr; ok = false;
  }
};

#ifndef EPI_HOST_ONLY
// template bytes per inflated byte, sampled from the file's first records (sum of l_seq over sum of record sizes: a
// PE150 Bismark / DRAGEN file gives ~0.35, where the worst-case bound is 0.4); 0.5 when the sample cannot be read
double pin_ratio_sample(const BamWindows &win) {
  std::vector<Block> head;
  size_t up = 0;
  for (size_t i = 0; i < win.blocks.size() && head.size() < 4; i++) { Block b = win.blocks[i]; b.upos = up; up += b.ulen; head.push_back(b); }
  std::vector<uint8_t> buf(up + 8);
  if (up < 16 || bgzf_inflate_range(win.file.p, head, 0, head.size(), buf.data(), 1) != EPI_OK || memcmp(buf.data(), "BAM\1", 4) != 0) return 0.5;
  size_t p = 8 + (size_t)rd32(buf.data() + 4);
  uint64_t nref = p + 4 <= up ? rd32(buf.data() + p) : 0;
  p += 4;
  while (nref > 0 && p + 4 <= up) { p += 8 + (size_t)rd32(buf.data() + p); nref--; }
  uint64_t bytes = 0, bases = 0;
  while (nref == 0 && p + 36 <= up) {
    const size_t bs = rd32(buf.data() + p);
    if (bs < 32 || p + 4 + bs > up) break;
    bytes += 4 + bs; bases += rd32(buf.data() + p + 4 + 16);
    p += 4 + bs;
  }
  return bytes >= 4096 && bases > 0 && bases < bytes ? (double)bases / (double)bytes : 0.5;
}

// the buffer pinned ahead: the file's inflated size times the sampled ratio plus 15 % (files below 8 MiB: none)
void pin_ahead_start(const BamWindows &win, PinAhead &pin) {
  const size_t total = win.inflated_size();
  if (total < ((size_t)8 << 20)) return;
  pin.cap = ((size_t)((double)total * pin_ratio_sample(win) * 1.15) + ((size_t)1 << 20) + 15) / 16 * 16;
  int cur_dev = -1;                                          // the caller's device, not device 0: every rank of a multi-GPU job pins under its own GPU
  if (hipGetDevice(&cur_dev) != hipSuccess) { (void)hipGetLastError(); cur_dev = -1; }
  pin.th = std::thread([&pin, cur_dev]() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && (cur_dev < 0 || hipSetDevice(cur_dev) == hipSuccess) &&
        hipHostMalloc(&pin.p, pin.cap, hipHostMallocDefault) == hipSuccess) pin.ok = true;
    else (void)hipGetLastError();
  });
}
#endif

// mates = "anywhere": a kept record of paired-end input, wherever its mate is.  Its QNAME is kept once per template (in
// the job's qmap); its CIGAR ops, packed query bytes and qualities go to the device arena at aoff, 4 * n_cig + 2 * l_seq
// bytes rounded up to 4.
struct Kept {
  uint32_t gid;                  // template id: the order of the templates' first kept records in the file
  int32_t tid, pos, mpos, isize;
  uint32_t rspan;                // reference length of the CIGAR (M D N = X), as apply_cigar sums it
  int64_t aoff;
  int32_t n_cig, l_seq;
  uint8_t cls, strand;           // flag & 0xC0 (merge order); XG's first letter
};
inline size_t kept_bytes(const Kept &k) { return ((size_t)k.n_cig * 4 + 2 * (size_t)k.l_seq + 3) & ~(size_t)3; }

// One call of preprocessBam: what its steps below share.
//
// genome != NULL (epi_preprocess_bam_genome): the records callMethylation would call are called on the GPU, window by
// window, into packed template bytes, and the packers read them in place of XG / XM -- the result is that of
// preprocessBam(callMethylation(path)) without the BAM in between.
//
// anyorder (epi_preprocess_bam_anyorder, mates = "anywhere"): paired-end records are paired through their QNAMEs wherever
// they lie in the file.  Per window, the kept records get their template ids and their CIGAR ops, packed query bytes and
// qualities go to a device arena; at the end of the file the host orders each template's records and lays out the rows,
// and assemble_templates.hip merges them on the GPU.
struct BamJob {
  epi_bam_options opt;
  epi_templates *out = nullptr;
  epi_engine *eng = nullptr;
  epi_genome *genome = nullptr;
  bool anyorder = false;
  size_t KT = 1;                                             // threads of the host loops
  BamWindows win;
  PinAhead pin;
  PackCtx ctx;
  // check_bam's findings
  bool paired = false, tMM = false;
  bool asm_mode = false;                                     // anyorder && paired-end short-read input
  StrandTag tag = TAG_XG;                                    // with a genome: the strand tag of the records to call
  // with a genome: the window's records to call
  CallSet CS;
  int64_t ncalled = 0;
#ifndef EPI_HOST_ONLY
  CallWork wk;
#endif
  // the templates, in file order
  Packed P;                                                  // the small columns of all templates (the bytes stay in `segs`)
  std::deque<Packed> segs;                                   // what the packing threads produced, kept until the ordered copy
  std::vector<const uint8_t *> src;                          // per template: its bytes inside a segment ...
  std::vector<int32_t> len;                                  // ... and how many
  size_t nrecs_total = 0;
  // mates = "anywhere"
  QnameMap qmap;
  std::vector<Kept> kept;
  std::vector<uint8_t> wk_keep;                              // per record of the window
  std::vector<char> wk_xg;
  std::vector<const char *> wk_xm;
  std::vector<uint32_t> wk_span, wk_ri;
  std::vector<uint64_t> wk_hash;
  size_t arena_used = 0;
  int stage_k = 0;
#ifndef EPI_HOST_ONLY
  DevBuf arena;                                              // sized by the file's inflated bytes: a kept record's inputs are
                                                             // smaller than the record
#endif
  std::vector<AsmRec> arec;                                  // kept records in merge order, template after template
  std::vector<int64_t> tpl_lo;                               // per template: its first record in arec (n + 1 entries)
  // the output
  std::vector<uint32_t> order;                               // output row -> template
  int64_t nbytes = 0;                                        // of all rows
  // EPIHIP_BAM_TIMING
  bool timing = false;
  double tm0 = 0, t_call = 0, t_pair = 0, t_upload = 0, t_group = 0;
  void lap(const char *what) { if (timing) { const double t = tnow(); fprintf(stderr, "[bam] %-10s %.3f s\n", what, t - tm0); tm0 = t; } }
};

// which of the window's records callMethylation would call, with its per-record checks
int select_calls(BamJob &J) {
  const double t0 = tnow();
  EPI_TRY(call_select(J.win.recs.begin(), J.win.recs.size(), J.tag, J.win.names, J.win.lens, J.KT, "epi_preprocess_bam", J.CS));
  J.t_call += tnow() - t0;
  return EPI_OK;
}

// The first window (at least 1024 records, or the whole file): endness, the kind of methylation tags, and whether the
// templates are assembled on the GPU.
int check_bam(BamJob &J) {
  const RecBuf &recs = J.win.recs;
  // with a genome, callMethylation's own checks come first: the strand tag, the header against the genome
  if (J.genome) {
    EPI_TRY(call_choose_tag(recs.begin(), recs.size(), nullptr, &J.tag));
    EPI_TRY(call_check_genome(J.genome, J.win.names, J.win.lens));
    EPI_TRY(select_calls(J));                                // (and its per-record checks over the whole window, before anything of it is packed)
  }
  // ---- .checkBam over the first 1024 records (src/rcpp_check_bam.cpp:40-50, R/internal.R:82-120) ----
  // (with a genome, as callMethylation's output would show them: a record to call carries XG and XM)
  size_t nrecs = 0, npaired = 0, ntempls = 0;
  bool tXG = false, tXM = false, tYD = false, tZS = false;
  const char *prevq = nullptr;
  for (const Rec &r : recs) {
    if (nrecs >= 1024) break;
    nrecs++;
    if (r.flag & 0x2) npaired++;
    const bool called = J.genome && J.CS.call[nrecs - 1];
    tXG |= called || has_tag(r, 'X', 'G'); tXM |= called || has_tag(r, 'X', 'M');
    tYD |= has_tag(r, 'Y', 'D'); tZS |= has_tag(r, 'Z', 'S');
    J.tMM |= has_tag(r, 'M', 'M') || has_tag(r, 'M', 'm');
    if (prevq && strcmp(prevq, r.qname) == 0) ntempls++;
    prevq = r.qname;
  }
  J.paired = npaired * 2 > nrecs;
  const bool sorted = ntempls > 0 && (ntempls >= nrecs / 2 || ntempls >= npaired / 2);
  if (nrecs == 0) return fail(EPI_ERR_ARG, "Empty file provided! Exiting");
  if (!tXG && tYD) return fail(EPI_ERR_ARG, "No XG tags found (though YD tags are there)! BWA-meth alignment? If so, make methylation calls using epialleleR::callMethylation. Exiting");
  if (!tXG && tZS) return fail(EPI_ERR_ARG, "No XG tags found (though ZS tags are there)! BSMAP alignment? If so, make methylation calls using epialleleR::callMethylation. Exiting");
  if (!tXM && tXG) return fail(EPI_ERR_ARG, "No XM tags found! Was methylation called successfully? If not, make methylation calls using epialleleR::callMethylation. Exiting");
  if (!J.tMM && !(tXG && tXM)) return fail(EPI_ERR_ARG, "No known methylation tags found! Exiting");
  if (J.paired && !sorted && !J.anyorder) return fail(EPI_ERR_ARG, "BAM file seems to be paired-end but not sorted by name! Please sort using 'samtools sort -n -o out.bam in.bam'. Exiting");
  if (J.opt.paired >= 0 && (J.opt.paired != 0) != J.paired) return fail(EPI_ERR_ARG, "Expected endness is different from detected! Exiting");
  J.asm_mode = J.anyorder && J.paired && !J.tMM;
#ifndef EPI_HOST_ONLY
  if (J.asm_mode) {
    EPI_HIP(hipSetDevice(J.eng->device));
    EPI_TRY(J.arena.ensure(J.win.inflated_size()));
  }
#endif
  return EPI_OK;
}

// with a genome: records [0, r_end), the ones about to be packed, are called on the GPU -- once, here
int call_window(BamJob &J, size_t r_end) {
  const double t0 = tnow();
  CallSet &CS = J.CS;
  EPI_TRY(call_pack_inputs(J.win.recs.begin(), r_end, J.KT, "epi_preprocess_bam", CS));
  const int64_t ncall = (int64_t)CS.crec.size();
  J.ncalled += ncall;
#ifndef EPI_HOST_ONLY
  if (!J.tMM)                                                // (the MM/ML packer reads no XG / XM)
    EPI_TRY(call_methylation_window(J.eng, J.genome, J.wk, CS.crec.data(), ncall, CS.cigar.data(), CS.ncig, CS.seq.data(),
                                    CS.nseq, CS.nxm, CALL_PACKED, CS.xm.data()));
#else
  return fail(EPI_ERR_NODEVICE, "epi_preprocess_bam_genome: this build has no device code");
#endif
  J.t_call += tnow() - t0;
  return EPI_OK;
}

// packs records [0, r_end) of the current window with the job's threads and appends the templates to P
int pack_window(BamJob &J, size_t r_end) {
  const RecBuf &recs = J.win.recs;
  std::vector<size_t> cut = even_cuts(r_end, r_end < 1024 ? 1 : J.KT);
  if (!J.tMM && J.paired)                                    // a template's records are neighbours with one QNAME
    for (size_t &c : cut)
      while (c > 0 && c < r_end && strcmp(recs[c].qname, recs[c - 1].qname) == 0) c++;
  std::vector<Packed> part(cut.size() - 1);
  EPI_TRY(fan_out(cut, "epi_preprocess_bam", "packing templates", [&](size_t k, size_t lo, size_t hi) -> int {
    Packed &q = part[k];
    q.off.push_back(0);
    size_t bases = 0;                                        // (one allocation instead of a doubling series per column)
    for (size_t i = lo; i < hi; i++) bases += (size_t)recs[i].l_seq;
    q.bytes.reserve(bases + bases / 8 + 4096);
    q.off.reserve(hi - lo + 2); q.rname.reserve(hi - lo + 1); q.strand.reserve(hi - lo + 1); q.start.reserve(hi - lo + 1);
    return J.tMM ? pack_mm(J.ctx, recs.begin(), lo, hi, q) : J.paired ? pack_pe(J.ctx, recs.begin(), lo, hi, q) : pack_se(J.ctx, recs.begin(), lo, hi, q);
  }));
  // the packed bytes stay where the threads wrote them (a segment per thread and window): only the small columns are
  // concatenated, and the final ordered copy reads the segments directly
  Packed &P = J.P;
  for (Packed &p : part) {
    J.segs.push_back(std::move(p));
    const Packed &q = J.segs.back();
    P.rname.insert(P.rname.end(), q.rname.begin(), q.rname.end());
    P.strand.insert(P.strand.end(), q.strand.begin(), q.strand.end());
    P.start.insert(P.start.end(), q.start.begin(), q.start.end());
    for (size_t i = 0; i + 1 < q.off.size(); i++) {
      J.src.push_back(q.bytes.data() + q.off[i]);
      J.len.push_back((int32_t)(q.off[i + 1] - q.off[i]));
    }
  }
  return EPI_OK;
}

#ifndef EPI_HOST_ONLY
// mates = "anywhere": the inputs of kept records [k0, kept.size()), all of this window, go to the device arena through
// the engine's two pinned staging buffers: filled by the threads while the copy stream drains the other one
int upload_kept(BamJob &J, size_t k0, size_t wbytes) {
  const RecBuf &recs = J.win.recs;
  const std::vector<Kept> &kept = J.kept;
  if (J.arena_used + wbytes > J.arena.cap) return fail(EPI_ERR_STATE, "epi_preprocess_bam_anyorder: device arena too small");
  auto fill = [&](size_t i, uint8_t *o) {                   // kept record k0 + i -> its arena bytes at o
    const Rec &r = recs[J.wk_ri[i]];
    if (r.n_cigar) memcpy(o, r.cigar, 4 * (size_t)r.n_cigar);
    o += 4 * (size_t)r.n_cigar;
    pack_query(r, J.wk_xm[J.wk_ri[i]], o);
    if (r.l_seq) memcpy(o + r.l_seq, r.qual, (size_t)r.l_seq);
  };
  const size_t nk = kept.size() - k0;
  for (size_t i = 0; i < nk;) {
    uint8_t *st;
    size_t cap;
    EPI_TRY(stage_buffer(J.eng, J.stage_k, &st, &cap));
    size_t j = i, bytes = 0;
    while (j < nk && bytes + kept_bytes(kept[k0 + j]) <= cap) bytes += kept_bytes(kept[k0 + j++]);
    if (j == i) {                                           // one record larger than a staging buffer: a copy of its own
      std::vector<uint8_t> big(kept_bytes(kept[k0 + i]));
      fill(i, big.data());
      EPI_HIP(hipMemcpy(J.arena.as<uint8_t>() + kept[k0 + i].aoff, big.data(), big.size(), hipMemcpyHostToDevice));
      i++;
      continue;
    }
    const int64_t a0 = kept[k0 + i].aoff;
    EPI_TRY(parallel_ranges(J.KT, j - i, "epi_preprocess_bam", [&](size_t lo, size_t hi) -> int {
      for (size_t x = i + lo; x < i + hi; x++) fill(x, st + (kept[k0 + x].aoff - a0));
      return EPI_OK;
    }));
    EPI_TRY(stage_send(J.eng, J.stage_k, J.arena.as<uint8_t>() + a0, bytes));
    J.stage_k ^= 1;
    i = j;
  }
  return EPI_OK;
}
#endif

// mates = "anywhere": the window's records [0, nrec): which are kept (pack_pe's filters and checks), their template ids,
// and their inputs queued for upload
int collect_window(BamJob &J, size_t nrec) {
  const double t0 = tnow();
  const RecBuf &recs = J.win.recs;
  const PackCtx &c = J.ctx;
  const uint16_t skip_flags_pe = c.skip_flags | 8;
  J.wk_keep.resize(nrec); J.wk_xg.resize(nrec); J.wk_xm.resize(nrec); J.wk_span.resize(nrec); J.wk_hash.resize(nrec);
  EPI_TRY(parallel_ranges(J.KT, nrec, "epi_preprocess_bam", [&](size_t lo, size_t hi) -> int {
    for (size_t ri = lo; ri < hi; ri++) {
      const Rec &r = recs[ri];
      J.wk_keep[ri] = 0;
      if ((r.flag & skip_flags_pe) || !(r.flag & 0x2) || (int)r.mapq < c.min_mapq) continue;   // pack_pe's filters
      char xg0;
      const char *xm;
      const uint8_t *pcall;
      if (!xg_xm(c, ri, r, &xg0, &xm, &pcall)) continue;
      uint32_t width, span = 0;
      EPI_TRY(use_record(c, r, xm, &width));
      EPI_TRY(apply_cigar(r, 0, [](uint32_t, uint32_t, uint32_t) {}, &span));
      J.wk_keep[ri] = 1; J.wk_xg[ri] = xg0; J.wk_xm[ri] = xm; J.wk_span[ri] = span;
      J.wk_hash[ri] = QnameMap::hash(r.qname);
    }
    return EPI_OK;
  }));
  const size_t k0 = J.kept.size();                           // ids in file order: the same for every nthreads
  J.wk_ri.clear();
  size_t wbytes = 0;
  for (size_t ri = 0; ri < nrec; ri++) {
    if (!J.wk_keep[ri]) continue;
    const Rec &r = recs[ri];
    Kept k;
    k.gid = J.qmap.find_or_add(r.qname, J.wk_hash[ri]);
    k.tid = r.tid; k.pos = r.pos; k.mpos = r.mpos; k.isize = r.isize; k.rspan = J.wk_span[ri];
    k.n_cig = (int32_t)r.n_cigar; k.l_seq = r.l_seq;
    k.cls = (uint8_t)(r.flag & 0xC0); k.strand = (uint8_t)(2 - (J.wk_xg[ri] == 'C' ? 1 : 0));
    k.aoff = (int64_t)(J.arena_used + wbytes);
    wbytes += kept_bytes(k);
    J.kept.push_back(k);
    J.wk_ri.push_back((uint32_t)ri);
  }
  const double t1 = tnow();
  J.t_pair += t1 - t0;
#ifndef EPI_HOST_ONLY
  EPI_TRY(upload_kept(J, k0, wbytes));
#else
  (void)k0;
#endif
  J.arena_used += wbytes;
  J.t_upload += tnow() - t1;
  return EPI_OK;
}

// mates = "anywhere": every template's records are known now.  Each one's records go in merge order (flag & 0xC0, then
// file order: READ1 before READ2), the first gives rname, start, width and strand, and the rest may widen it -- pack_pe's
// rules and errors on G(F), without touching a byte (the kernel merges them once the rows have their places).
int group_templates(BamJob &J) {
  std::vector<Kept> &kept = J.kept;
  std::vector<int64_t> &tpl_lo = J.tpl_lo;
  const size_t G = J.qmap.size(), NK = kept.size();
  tpl_lo.assign(G + 1, 0);
  for (const Kept &k : kept) tpl_lo[k.gid + 1]++;
  for (size_t g = 0; g < G; g++) tpl_lo[g + 1] += tpl_lo[g];
  std::vector<uint32_t> mo(NK);                             // kept records by template, in file order (a stable counting sort)
  {
    std::vector<int64_t> cur(tpl_lo.begin(), tpl_lo.end() - 1);
    for (size_t i = 0; i < NK; i++) mo[(size_t)cur[kept[i].gid]++] = (uint32_t)i;
  }
  J.arec.resize(NK);
  J.P.rname.reserve(G); J.P.strand.reserve(G); J.P.start.reserve(G); J.len.reserve(G);
  for (size_t g = 0; g < G; g++) {
    uint32_t *m = mo.data() + tpl_lo[g], nm = (uint32_t)(tpl_lo[g + 1] - tpl_lo[g]);
    for (uint32_t a = 1; a < nm; a++)                       // (stable insertion sort by flag & 0xC0: a template has few records)
      for (uint32_t b = a; b > 0 && kept[m[b]].cls < kept[m[b - 1]].cls; b--) std::swap(m[b], m[b - 1]);
    const Kept &f = kept[m[0]];
    const int t_start = f.pos < f.mpos ? f.pos : f.mpos;                                     // :92-93
    if (f.isize == INT32_MIN) return fail(EPI_ERR_ARG, "corrupt BAM record %s: template length", J.qmap.name((uint32_t)g));
    int t_width = f.isize < 0 ? -f.isize : f.isize;                                          // :94
    for (uint32_t a = 0; a < nm; a++) {
      const Kept &k = kept[m[a]];
      if (k.pos < t_start) return fail(EPI_ERR_ARG, "corrupt BAM record %s: starts before its template", J.qmap.name((uint32_t)g));
      const uint32_t dest0 = (uint32_t)(k.pos - t_start), dest_end = dest0 + k.rspan;     // :118 (apply_cigar's sum)
      if (dest_end > 0x7FFFFFFFu) return fail(EPI_ERR_ARG, "corrupt BAM record %s: template too wide", J.qmap.name((uint32_t)g));
      if (t_width < (int)dest_end) t_width = (int)dest_end;                                  // :151
      AsmRec &x = J.arec[(size_t)tpl_lo[g] + a];
      x.arena_off = k.aoff; x.dest0 = (int32_t)dest0; x.n_cig = k.n_cig; x.l_seq = k.l_seq; x.pad = 0;
    }
    J.P.rname.push_back(f.tid + 1);                                                          // :61-69
    J.P.strand.push_back(f.strand);
    J.P.start.push_back(t_start + J.ctx.trim5 + 1);
    const int keep = t_width - (J.ctx.trim5 + J.ctx.trim3);
    J.len.push_back(keep > 0 ? keep : 0);
  }
  std::vector<Kept>().swap(kept);
  return EPI_OK;
}

// ---- templid := 0..N-1 ; setorder(rname, start) -- stable (R/internal.R:193-195) ----
int sort_templates(BamJob &J) {
  const Packed &P = J.P;
  const size_t n = P.rname.size();
  std::vector<uint32_t> &order = J.order;
  order.resize(n);
  std::iota(order.begin(), order.end(), 0u);
  auto less = [&](uint32_t a, uint32_t b) {
    if (P.rname[a] != P.rname[b]) return P.rname[a] < P.rname[b];
    return P.start[a] < P.start[b];
  };
  // stable: ranges sorted by the threads, then merged pairwise (std::inplace_merge keeps equal keys in order)
  size_t K = 1;
  while (K * 2 <= J.KT && n / (K * 2) >= 65536) K *= 2;
  const std::vector<size_t> cut = even_cuts(n, K);
  EPI_TRY(fan_out(cut, "epi_preprocess_bam", "sorting templates", [&](size_t, size_t lo, size_t hi) -> int {
    std::stable_sort(order.begin() + lo, order.begin() + hi, less);
    return EPI_OK;
  }));
  for (size_t w = 1; w < K; w *= 2) {                        // merge runs of w ranges
    std::vector<std::thread> th;
    for (size_t k = 0; k + w < K; k += 2 * w) {
      const size_t lo = cut[k], mid = cut[k + w], hi = cut[k + 2 * w < K ? k + 2 * w : K];
      th.emplace_back([&, lo, mid, hi]() { std::inplace_merge(order.begin() + lo, order.begin() + mid, order.begin() + hi, less); });
    }
    for (auto &t : th) t.join();
  }
  return EPI_OK;
}

// the output columns: the bytes in the buffer pinned ahead where it fits, and every row's offset
int allocate_output(BamJob &J) {
  epi_templates *out = J.out;
  const size_t n = J.order.size();
  size_t nbytes = 0;
  for (size_t i = 0; i < n; i++) nbytes += (size_t)J.len[i];
  size_t cap = (nbytes + 15) / 16 * 16 + 64;
  void *xmp = nullptr;
#ifdef EPI_HOST_ONLY
  xmp = malloc(cap); out->pinned = 0;                      // host-only sanitizer build (`make asan`)
#else
  PinAhead &pin = J.pin;
  pin.wait();
  // the buffer pinned while the file was being read -- unless it turned out too small, or more than a quarter larger
  // than needed (page-locked memory stays pinned for the life of the templates: then the exact size is allocated)
  if (pin.ok && pin.cap >= cap && pin.cap <= cap + cap / 4 + ((size_t)4 << 20)) {
    xmp = pin.p; out->pinned = 1;
    pin.p = nullptr; pin.ok = false;
  } else {
    pin.release();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && hipHostMalloc(&xmp, cap, hipHostMallocDefault) == hipSuccess) out->pinned = 1;
    else { (void)hipGetLastError(); xmp = malloc(cap); out->pinned = 0; }
  }
#endif
  out->xm = (uint8_t *)xmp;
  out->off = (int64_t *)malloc((n + 1) * sizeof(int64_t));
  out->rname = (int32_t *)malloc((n + 1) * sizeof(int32_t));
  out->strand = (int32_t *)malloc((n + 1) * sizeof(int32_t));
  out->start = (int32_t *)malloc((n + 1) * sizeof(int32_t));
  out->target_names = (char **)calloc(J.win.names.size() + 1, sizeof(char *));
  if (!out->xm || !out->off || !out->rname || !out->strand || !out->start || !out->target_names) {
    epi_templates_free(out);
    return fail(EPI_ERR_NOMEM, "epi_preprocess_bam: out of host memory");
  }
  int64_t w = 0;
  for (size_t i = 0; i < n; i++) { out->off[i] = w; w += J.len[J.order[i]]; }
  out->off[n] = w;
  J.nbytes = w;
  return EPI_OK;
}

// the ordered copy, by ranges of output rows (mates = "anywhere": the small columns only, the GPU writes the bytes)
int copy_ordered(BamJob &J) {
  epi_templates *out = J.out;
  const size_t n = J.order.size();
  return fan_out(even_cuts(n, n < 4096 ? 1 : J.KT), "epi_preprocess_bam", "copying templates", [&](size_t, size_t lo, size_t hi) -> int {
    for (size_t i = lo; i < hi; i++) {
      const uint32_t t = J.order[i];
      if (J.len[t] && !J.asm_mode) memcpy(out->xm + out->off[i], J.src[t], (size_t)J.len[t]);
      out->rname[i] = J.P.rname[t]; out->strand[i] = J.P.strand[t]; out->start[i] = J.P.start[t];
    }
    return EPI_OK;
  });
}

// mates = "anywhere": the rows, merged on the GPU in their output slots
int assemble_on_gpu(BamJob &J) {
#ifndef EPI_HOST_ONLY
  const size_t n = J.order.size();
  std::vector<AsmTpl> tpl(n);
  int64_t qbytes = 0;
  for (size_t i = 0; i < n; i++) {
    const uint32_t t = J.order[i];
    AsmTpl &x = tpl[i];
    x.out_off = J.out->off[i]; x.rec_lo = J.tpl_lo[t]; x.nrec = (int32_t)(J.tpl_lo[t + 1] - J.tpl_lo[t]); x.keep = J.len[t];
    x.q_off = 0;
    if (J.len[t] > kAsmLdsWidth) { x.q_off = qbytes; qbytes += J.len[t]; }
  }
  const double t0 = tnow();
  EPI_HIP(hipStreamSynchronize(J.eng->copy_stream));         // (the arena's last uploads)
  J.t_upload += tnow() - t0;
  const uint8_t q0 = (uint8_t)(J.ctx.min_baseq - (J.ctx.min_baseq > 0 ? 1 : 0));   // src/rcpp_read_bam.cpp:30,57
  double t_kernel = 0, t_d2h = 0;
  EPI_TRY(assemble_templates(J.eng, J.arena.as<uint8_t>(), tpl.data(), (int64_t)n, J.arec.data(), (int64_t)J.arec.size(), q0,
                             J.ctx.trim5, J.nbytes, qbytes, J.out->xm, &t_kernel, &t_d2h));
  if (J.timing)
    fprintf(stderr, "[bam] (anywhere: inflate %.3f s, parse %.3f s, pairing %.3f s, upload %.3f s, grouping %.3f s, "
                    "kernel %.3f s, D2H %.3f s)\n", J.win.t_inflate, J.win.t_parse, J.t_pair, J.t_upload, J.t_group, t_kernel, t_d2h);
#else
  (void)J;
#endif
  return EPI_OK;
}

void finish(BamJob &J, int64_t *ncalled_out) {
  epi_templates *out = J.out;
  const std::vector<std::string> &names = J.win.names;
  // 0xFB padding up to the 16-byte boundary the kernels may read to, plus a little (a buffer pinned ahead can be much
  // larger than the templates: its tail stays untouched and is not part of xm_capacity)
  const size_t padded = ((size_t)J.nbytes + 15) / 16 * 16 + 64;
  memset(out->xm + J.nbytes, 0xFB, padded - (size_t)J.nbytes);
  J.lap("sort+copy");
  out->n = (int64_t)J.order.size();
  out->nbytes = J.nbytes;
  out->xm_capacity = (int64_t)padded;
  out->nrecs = (int64_t)J.nrecs_total;
  if (ncalled_out) *ncalled_out = J.ncalled;
  out->paired = J.paired ? 1 : 0;
  out->n_targets = (int32_t)names.size();
  for (size_t i = 0; i < names.size(); i++) out->target_names[i] = strdup(names[i].c_str());
}

// option defaults, the thread cap and what the packers read of them
int set_options(BamJob &J, const epi_bam_options *opt_in) {
  epi_bam_options &opt = J.opt;
  if (opt_in) opt = *opt_in;
  else { memset(&opt, 0, sizeof(opt)); opt.skip_secondary = opt.skip_qcfail = opt.skip_supplementary = 1; opt.paired = -1; opt.nthreads = 1; opt.min_prob = -1; opt.highest_prob = 1; }
  if (opt.trim5 < 0 || opt.trim3 < 0) return fail(EPI_ERR_ARG, "trim must be non-negative");
  J.KT = thread_cap(opt.nthreads);
  uint16_t skip_flags = 4;
  if (opt.skip_secondary) skip_flags |= 256;
  if (opt.skip_qcfail) skip_flags |= 512;
  if (opt.skip_duplicates) skip_flags |= 1024;
  if (opt.skip_supplementary) skip_flags |= 2048;
  J.ctx = PackCtx{skip_flags, opt.min_mapq, opt.min_baseq, opt.min_prob, opt.highest_prob, opt.trim5, opt.trim3, 0, nullptr};
  J.timing = epi::options().bam_timing != 0;
  J.tm0 = tnow();
  return EPI_OK;
}

int preprocess_impl(const char *path, const epi_bam_options *opt_in, epi_templates *out, epi_engine *eng,
                    epi_genome *genome, int64_t *ncalled_out, bool anyorder) {
  BamJob J;
  J.out = out; J.eng = eng; J.genome = genome; J.anyorder = anyorder;
  EPI_TRY(set_options(J, opt_in));
  BamWindows &win = J.win;
  // with a genome, the header messages are callMethylation's: it reads the file first
  EPI_TRY(win.open(path, J.opt.window_kib, (size_t)256 << 20, J.opt.nthreads, genome ? "Unable to read input BAM header" : "Unable to read BAM header"));
#ifndef EPI_HOST_ONLY
  pin_ahead_start(win, J.pin);
#endif
  bool checked = false;
  for (;;) {
    bool final;
    EPI_TRY(win.next(&final));
    if (!checked) {
      if (win.recs.size() < 1024 && !final) { win.keep_all(); continue; }   // .checkBam looks at the first 1024 records
      J.lap("index");
      J.ctx.n_ref = win.names.size();
      J.ctx.calls = genome ? &J.CS : nullptr;
      EPI_TRY(check_bam(J));
      checked = true;
    } else if (genome) {
      EPI_TRY(select_calls(J));
    }
    // paired-end: the records of the window's last QNAME wait for the next window (their mate may be in it)
    size_t r_end = win.recs.size();
    if (!final && J.paired && !J.tMM && !J.asm_mode && r_end > 0) {
      const char *lastq = win.recs[r_end - 1].qname;
      while (r_end > 0 && strcmp(win.recs[r_end - 1].qname, lastq) == 0) r_end--;
      if (r_end == 0) { win.keep_all(); continue; }          // one template fills the window: read on
    }
    if (genome) EPI_TRY(call_window(J, r_end));
    if (J.asm_mode) EPI_TRY(collect_window(J, r_end));
    else EPI_TRY(pack_window(J, r_end));
    J.nrecs_total += r_end;
    win.consume(r_end);
    if (final) break;
  }
  const double t_g0 = tnow();
  if (J.asm_mode) EPI_TRY(group_templates(J));
  if (!J.tMM && J.paired && J.P.rname.empty()) {             // the reference pushes its (never opened) template all the same, :155
    J.P.rname.push_back(1); J.P.strand.push_back(0); J.P.start.push_back(J.ctx.trim5 + 1); J.src.push_back(nullptr); J.len.push_back(0);
    if (J.asm_mode) J.tpl_lo.push_back(J.tpl_lo.back());
  }
  win.release();
  J.t_group = tnow() - t_g0;
  J.lap("pack");
  if (J.timing && genome) fprintf(stderr, "[bam] (of which call selection, inputs and GPU %.3f s)\n", J.t_call);
  EPI_TRY(sort_templates(J));
  EPI_TRY(allocate_output(J));
  EPI_TRY(copy_ordered(J));
  if (J.asm_mode) EPI_TRY(assemble_on_gpu(J));
  finish(J, ncalled_out);
  return EPI_OK;
}

// the three preprocessBam entry points: nothing may unwind through the C boundary, and a failed call leaves *out empty
int preprocess_entry(const char *path, const epi_bam_options *opt_in, epi_templates *out, epi_engine *eng, epi_genome *genome,
                     int64_t *ncalled, bool anyorder) {
  int rc;
  try {
    rc = preprocess_impl(path, opt_in, out, eng, genome, ncalled, anyorder);
  } catch (const std::bad_alloc &) {
    rc = fail(EPI_ERR_NOMEM, "epi_preprocess_bam: out of host memory");
  } catch (...) {
    rc = fail(EPI_ERR_ARG, "epi_preprocess_bam: unexpected failure while reading %s", path);
  }
  if (rc != EPI_OK) { epi_templates_free(out); if (ncalled) *ncalled = 0; }
  return rc;
}

// ---- callMethylation: BAM in, BAM out (rcpp_call_methylation_genome, src/rcpp_call_methylation.cpp:27-177, with
// .callMethylation's tag choice, R/internal.R:405-432) ------------------------------------------------------------------
// The file goes through the reader's windows (block scan, parallel inflate and parse_record).  Per window the
// host picks the records to call (mapped, carrying the strand tag, no XM yet), checks them and packs their CIGAR and
// SEQ; the GPU computes their XM bytes (call_methylation.hip); the records are then written out in input order -- the
// called ones with XG (when the tag was YD or ZS) and XM appended -- and deflated into BGZF blocks by `nthreads`
// threads.  Host memory is bounded by the window (inflated bytes, the records written out, the packed call inputs).
#ifndef EPI_HOST_ONLY
struct Window {                       // what one window's records turn into
  std::vector<uint64_t> out_off;      // per record: where its output starts (n + 1 entries)
  std::vector<uint8_t> out;
};

// the window's records, in input order, with the new tags appended (bam_aux_append / bam_aux_update_str)
int call_splice(BamWindows &win, const CallSet &S, StrandTag tag, size_t K, Window &W) {
  const size_t nrec = win.recs.size();
  W.out.resize((size_t)W.out_off[nrec]);
  return parallel_ranges(K, nrec, "epi_call_methylation", [&](size_t lo, size_t hi) -> int {
    for (size_t i = lo; i < hi; i++) {
      const uint8_t *src = win.record(i);
      const uint32_t bs = rd32(src);
      uint8_t *o = W.out.data() + W.out_off[i];
      if (!S.call[i]) { memcpy(o, src, 4 + (size_t)bs); continue; }
      const uint64_t nb = W.out_off[i + 1] - W.out_off[i] - 4;
      o[0] = (uint8_t)nb; o[1] = (uint8_t)(nb >> 8); o[2] = (uint8_t)(nb >> 16); o[3] = (uint8_t)(nb >> 24);
      memcpy(o + 4, src + 4, bs);
      o += 4 + (size_t)bs;
      if (tag != TAG_XG) {
        const bool ga = S.s_meth[i] == 'G';
        const uint8_t xg[6] = {'X', 'G', 'Z', (uint8_t)(ga ? 'G' : 'C'), (uint8_t)(ga ? 'A' : 'T'), 0};
        memcpy(o, xg, 6);
        o += 6;
      }
      o[0] = 'X'; o[1] = 'M'; o[2] = 'Z';
      const Rec &r = win.recs[i];
      if (r.l_seq) memcpy(o + 3, S.xm.data() + S.crec[(size_t)S.call_idx[i]].xm_off, (size_t)r.l_seq);
      o[3 + r.l_seq] = 0;
    }
    return EPI_OK;
  });
}

int call_impl(epi_engine *eng, const char *in_path, const char *out_path, epi_genome *g, const char *force_tag,
              int nthreads, int32_t window_kib, int64_t *nrecs_out, int64_t *ncalled_out) {
  BamWindows win;
  EPI_TRY(win.open(in_path, window_kib, (size_t)64 << 20, nthreads, "Unable to read input BAM header"));
  const size_t K = thread_cap(nthreads);
  bool checked = false;
  StrandTag tag = TAG_XG;
  BgzfWriter out;
  CallWork wk;
  CallSet S;
  Window W;
  int64_t nrecs = 0, ncalled = 0;
  // phase times (EPIHIP_BAM_TIMING, as for the reader): inflate + index, host preparation, GPU, splice, deflate + write
  const bool timing = epi::options().bam_timing != 0;
  double t_phase[5] = {0, 0, 0, 0, 0}, t_mark = tnow();
  auto lap = [&](int k) { const double t = tnow(); t_phase[k] += t - t_mark; t_mark = t; };

  for (;;) {
    bool final;
    EPI_TRY(win.next(&final));
    const Rec *recs = win.recs.begin();
    const size_t nrec = win.recs.size();
    lap(0);
    if (!checked) {
      if (nrec < 1024 && !final) { win.keep_all(); continue; }   // .checkBam looks at the first 1024 records
      EPI_TRY(call_choose_tag(recs, nrec, force_tag, &tag));
      // ---- the output and the header check (src/rcpp_call_methylation.cpp:41-72) ----
      EPI_TRY(out.open(out_path));
      EPI_TRY(call_check_genome(g, win.names, win.lens));
      EPI_TRY(out.write(win.header(), win.header_size(), nthreads));   // the input header, verbatim
      checked = true;
    }
    // ---- which records are called, and how large each one is written out ----
    EPI_TRY(call_select(recs, nrec, tag, win.names, win.lens, K, "epi_call_methylation", S));
    W.out_off.resize(nrec + 1);
    W.out_off[0] = 0;
    for (size_t i = 0; i < nrec; i++) {
      const uint64_t bs = rd32(win.record(i));
      W.out_off[i + 1] = W.out_off[i] + 4 + bs + (S.call[i] ? (tag == TAG_XG ? 0 : 6) + 4 + (uint64_t)recs[i].l_seq : 0);
    }
    // ---- the packed inputs of the called records ----
    EPI_TRY(call_pack_inputs(recs, nrec, K, "epi_call_methylation", S));
    const int64_t ncall = (int64_t)S.crec.size();
    lap(1);
    // ---- the GPU: XM of every called record ----
    EPI_TRY(call_methylation_window(eng, g, wk, S.crec.data(), ncall, S.cigar.data(), S.ncig, S.seq.data(), S.nseq, S.nxm,
                                    CALL_XM, S.xm.data()));
    lap(2);
    EPI_TRY(call_splice(win, S, tag, K, W));
    lap(3);
    EPI_TRY(out.write(W.out.data(), W.out.size(), nthreads));
    lap(4);
    nrecs += (int64_t)nrec;
    ncalled += ncall;
    win.consume(nrec);
    if (final) break;
  }
  if (!checked) return fail(EPI_ERR_ARG, "Empty file provided! Exiting");
  EPI_TRY(out.close());
  lap(4);
  if (timing)
    fprintf(stderr, "[call] inflate+index %.3f s  prepare %.3f s  gpu %.3f s  splice %.3f s  deflate+write %.3f s\n",
            t_phase[0], t_phase[1], t_phase[2], t_phase[3], t_phase[4]);
  *nrecs_out = nrecs;
  *ncalled_out = ncalled;
  return EPI_OK;
}
#endif  // EPI_HOST_ONLY

}  // namespace

extern "C" {

void epi_templates_free(epi_templates *t) {
  if (!t) return;
#ifdef EPI_HOST_ONLY
  free(t->xm);                                             // (sanitizer build: no HIP runtime, the bytes came from malloc)
#else
  if (t->xm) { if (t->pinned) (void)hipHostFree(t->xm); else free(t->xm); }
#endif
  free(t->off); free(t->rname); free(t->strand); free(t->start);
  if (t->target_names) { for (int32_t i = 0; i < t->n_targets; i++) free(t->target_names[i]); free(t->target_names); }
  memset(t, 0, sizeof(*t));
}

int epi_preprocess_bam(const char *path, const epi_bam_options *opt_in, epi_templates *out) {
  if (!path || !out) return fail(EPI_ERR_ARG, "epi_preprocess_bam: NULL argument");
  memset(out, 0, sizeof(*out));
  return preprocess_entry(path, opt_in, out, nullptr, nullptr, nullptr, false);
}

int epi_preprocess_bam_genome(epi_engine *eng, const char *path, const epi_bam_options *opt_in, epi_genome *g,
                              epi_templates *out, int64_t *ncalled) {
  if (!path || !out || !g || !ncalled) return fail(EPI_ERR_ARG, "epi_preprocess_bam_genome: NULL argument");
  memset(out, 0, sizeof(*out));
  *ncalled = 0;
#ifdef EPI_HOST_ONLY
  (void)eng; (void)opt_in;
  return fail(EPI_ERR_NODEVICE, "epi_preprocess_bam_genome: the calls are made on the GPU; this build has no device code");
#else
  if (!eng) EPI_TRY(epi_default_engine(&eng));               // no device: fails here, before the file is read
  return preprocess_entry(path, opt_in, out, eng, g, ncalled, false);
#endif
}

int epi_preprocess_bam_anyorder(epi_engine *eng, const char *path, const epi_bam_options *opt_in, epi_templates *out) {
  if (!path || !out) return fail(EPI_ERR_ARG, "epi_preprocess_bam_anyorder: NULL argument");
  memset(out, 0, sizeof(*out));
#ifdef EPI_HOST_ONLY
  (void)eng; (void)opt_in;
  return fail(EPI_ERR_NODEVICE, "epi_preprocess_bam_anyorder: templates are assembled on the GPU; this build has no device code");
#else
  if (!eng) EPI_TRY(epi_default_engine(&eng));               // no device: fails here, before the file is read
  return preprocess_entry(path, opt_in, out, eng, nullptr, nullptr, true);
#endif
}

#ifndef EPI_HOST_ONLY
int epi_call_methylation_windowed(epi_engine *eng, const char *in_path, const char *out_path, epi_genome *g, const char *tag,
                                  int nthreads, int32_t window_kib, int64_t *nrecs, int64_t *ncalled) {
  if (!in_path || !out_path || !g || !nrecs || !ncalled) return fail(EPI_ERR_ARG, "epi_call_methylation: NULL argument");
  if (tag && strcmp(tag, "XG") != 0 && strcmp(tag, "YD") != 0 && strcmp(tag, "ZS") != 0)
    return fail(EPI_ERR_ARG, "epi_call_methylation: tag must be XG, YD or ZS");
  *nrecs = 0; *ncalled = 0;
  if (!eng) EPI_TRY(epi_default_engine(&eng));               // no device: fails here, before any file is touched
  int rc;
  bool wrote = false;
  try {
    struct stat st;
    wrote = !(*out_path && stat(out_path, &st) == 0);        // (a partial output is removed only if this call created it)
    rc = call_impl(eng, in_path, out_path, g, tag, nthreads, window_kib, nrecs, ncalled);
  } catch (const std::bad_alloc &) {
    rc = fail(EPI_ERR_NOMEM, "epi_call_methylation: out of host memory");
  } catch (...) {
    rc = fail(EPI_ERR_ARG, "epi_call_methylation: unexpected failure while reading %s", in_path);
  }
  if (rc != EPI_OK) {
    *nrecs = 0; *ncalled = 0;
    if (wrote && *out_path) (void)unlink(out_path);
  }
  return rc;
}

int epi_call_methylation(epi_engine *eng, const char *in_path, const char *out_path, epi_genome *g, int nthreads,
                         int64_t *nrecs, int64_t *ncalled) {
  return epi_call_methylation_windowed(eng, in_path, out_path, g, nullptr, nthreads, 0, nrecs, ncalled);
}
#endif  // EPI_HOST_ONLY

}  // extern "C"


// ---- whole-file inflate for the other host readers (vcf_reader.cpp) ----------------------------------------------
// BGZF through the same block scan and parallel inflate as the BAM reader; a gzip file that is not BGZF through zlib
// (any number of members); anything else is returned as it is.
int epi::read_text_file(const char *path, std::vector<uint8_t> &out, int nthreads) {
  out.clear();
  FileView file;
  if (open_file(path, file) != EPI_OK) return fail(EPI_ERR_ARG, "Unable to open file for reading: %s", path);
  if (file.n < 2 || file.p[0] != 0x1f || file.p[1] != 0x8b) { out.assign(file.p, file.p + file.n); return EPI_OK; }
  std::vector<Block> blocks;
  if (bgzf_scan(file.p, file.n, blocks) == EPI_OK) {
    size_t u = 0;
    for (Block &b : blocks) { b.upos = u; u += b.ulen; }
    out.resize(u);
    return bgzf_inflate_range(file.p, blocks, 0, blocks.size(), out.data(), nthreads);
  }
  z_stream zs;
  memset(&zs, 0, sizeof(zs));
  if (inflateInit2(&zs, 15 + 32) != Z_OK) return fail(EPI_ERR_NOMEM, "inflateInit2 failed");
  zs.next_in = const_cast<Bytef *>(file.p);
  zs.avail_in = (uInt)file.n;                                // (a gzip file that is not BGZF: small, below 4 GiB)
  uint8_t buf[1 << 16];
  int rc = Z_OK;
  for (;;) {
    zs.next_out = buf;
    zs.avail_out = sizeof(buf);
    rc = inflate(&zs, Z_NO_FLUSH);
    out.insert(out.end(), buf, buf + (sizeof(buf) - zs.avail_out));
    if (rc == Z_STREAM_END) {
      if (zs.avail_in == 0) break;
      if (inflateReset(&zs) != Z_OK) { rc = Z_DATA_ERROR; break; }   // the next member
      continue;
    }
    if (rc != Z_OK) break;
  }
  inflateEnd(&zs);
  if (rc != Z_STREAM_END) return fail(EPI_ERR_ARG, "corrupt gzip file: %s", path);
  return EPI_OK;
}
