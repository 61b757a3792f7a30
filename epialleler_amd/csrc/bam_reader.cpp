// The BAM reader (bam_reader.hpp), without HTSlib: BGZF is a series of gzip members whose compressed size is in the
// BC extra field (SAM spec 4.1), so the blocks are located without inflating (the file is mmap-ed) and inflated in
// parallel by worker threads, window by window (a record or template that straddles a window seam is carried over);
// BAM records have a fixed layout (SAM spec 4.2) and are validated before use.
#include <zlib.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <atomic>
#include "bam_reader.hpp"

namespace epi {
namespace bam {

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
static const FastInflate &fast_inflate() { static const FastInflate f; return f; }

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

// ---- BamWindows --------------------------------------------------------------------------------------------------------
int BamWindows::open(const char *path, int32_t window_kib, size_t default_window, int nthreads, const char *hdr_msg) {
  window_ = window_kib > 0 ? (size_t)window_kib * 1024 : default_window;
  nthreads_ = nthreads;
  hdr_msg_ = hdr_msg;
  EPI_TRY(open_file(path, file));
  return bgzf_scan(file.p, file.n, blocks);
}

size_t BamWindows::inflated_size() const {
  size_t total = 0;
  for (const Block &b : blocks) total += b.ulen;
  return total;
}

int BamWindows::next(bool *final) {
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

void BamWindows::consume(size_t r_end) {
  const size_t keep_from = r_end < recs.size() ? roff_[r_end] : end_;
  carry_ = buf_.size() - keep_from;
  if (carry_) memmove(buf_.data(), buf_.data() + keep_from, carry_);
  hdr_end_ = 0;                                            // (the header is gone from the buffer)
  recs.clear();
}

// BAM header: magic, text, reference names and lengths.  *complete: all of it is in the buffer, up to hdr_end_.
int BamWindows::parse_header(bool *complete) {
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
size_t BamWindows::index_records(size_t kb, std::vector<Span> &spans) {
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

int BamWindows::parse_records(const std::vector<Span> &spans, size_t nrec) {
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

}  // namespace bam
}  // namespace epi

using namespace epi::bam;

// ---- whole-file inflate for the other host readers (vcf_reader.cpp, genome.cpp) ----------------------------------
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
