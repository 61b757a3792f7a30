// BGZF output (SAM spec 4.1), as HTSlib writes it: blocks of at most 0xff00 input bytes, each a gzip member with the
// BC extra field (its total size - 1) and the CRC32 / size of its input, then the standard 28-byte end-of-file block.
// Blocks are deflated at level 6 by `nthreads` threads and written in order.  libdeflate's compressor is used when
// libdeflate.so.0 can be loaded at run time (as the reader's FastInflate does), zlib otherwise.
#include <dlfcn.h>
#include <stdio.h>
#include <string.h>
#include <zlib.h>
#include <atomic>
#include <thread>
#include <vector>
#include "common.hpp"

using namespace epi;

namespace {

constexpr size_t kBlockIn = 0xff00;                 // input bytes per block (HTSlib's BGZF_BLOCK_SIZE)
constexpr size_t kBlockMax = 0x10000;               // a block, header and trailer included
constexpr size_t kHeader = 18, kTrailer = 8;
constexpr int kLevel = 6;

struct FastDeflate {
  void *(*alloc)(int) = nullptr;
  size_t (*run)(void *, const void *, size_t, void *, size_t) = nullptr;
  void (*release)(void *) = nullptr;
  FastDeflate() {
    if (epi::options().no_libdeflate) return;
    void *h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
    alloc = reinterpret_cast<void *(*)(int)>(dlsym(h, "libdeflate_alloc_compressor"));
    run = reinterpret_cast<size_t (*)(void *, const void *, size_t, void *, size_t)>(dlsym(h, "libdeflate_deflate_compress"));
    release = reinterpret_cast<void (*)(void *)>(dlsym(h, "libdeflate_free_compressor"));
    if (!alloc || !run || !release) { alloc = nullptr; run = nullptr; release = nullptr; }
  }
  bool ok() const { return run != nullptr; }
};
const FastDeflate &fast_deflate() { static const FastDeflate f; return f; }

inline void wr16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
inline void wr32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// one compressing thread's state: libdeflate's compressor or a zlib stream, reused block after block
struct Deflater {
  void *ld = nullptr;
  z_stream zs;
  bool z_ok = false;
  Deflater() {
    const FastDeflate &fd = fast_deflate();
    if (fd.ok()) ld = fd.alloc(kLevel);
    if (!ld) {
      memset(&zs, 0, sizeof(zs));
      z_ok = deflateInit2(&zs, kLevel, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) == Z_OK;
    }
  }
  ~Deflater() {
    if (ld) fast_deflate().release(ld);
    if (z_ok) deflateEnd(&zs);
  }
  // raw deflate of in[0, n) into out (capacity cap); the compressed size, 0 on failure
  size_t run(const uint8_t *in, size_t n, uint8_t *out, size_t cap) {
    if (ld) return fast_deflate().run(ld, in, n, out, cap);
    if (!z_ok || deflateReset(&zs) != Z_OK) return 0;
    zs.next_in = const_cast<Bytef *>(in); zs.avail_in = (uInt)n;
    zs.next_out = out; zs.avail_out = (uInt)cap;
    if (deflate(&zs, Z_FINISH) != Z_STREAM_END) return 0;
    return cap - zs.avail_out;
  }
};

// block = header, compressed payload, CRC32, input size; returns its size (0: failure)
size_t make_block(Deflater &d, const uint8_t *in, size_t n, uint8_t *blk) {
  static const uint8_t hdr[kHeader - 2] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
  memcpy(blk, hdr, sizeof(hdr));
  size_t c = d.run(in, n, blk + kHeader, kBlockMax - kHeader - kTrailer);
  if (c == 0) return 0;
  const size_t total = kHeader + c + kTrailer;
  wr16(blk + 16, (uint32_t)(total - 1));
  wr32(blk + kHeader + c, (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, (uInt)n));
  wr32(blk + kHeader + c + 4, (uint32_t)n);
  return total;
}

}  // namespace

namespace epi {

BgzfWriter::~BgzfWriter() { if (f_) fclose(static_cast<FILE *>(f_)); }

int BgzfWriter::open(const char *path) {
  f_ = path && *path ? fopen(path, "wb") : nullptr;
  if (!f_) return fail(EPI_ERR_ARG, "Unable to open output BAM file for writing");   // src/rcpp_call_methylation.cpp:43
  return EPI_OK;
}

int BgzfWriter::write(const uint8_t *data, size_t n, int nthreads) {
  if (!f_) return fail(EPI_ERR_STATE, "BGZF writer is not open");
  const size_t nblk = (n + kBlockIn - 1) / kBlockIn;
  if (nblk == 0) return EPI_OK;
  // a batch of blocks at a time: the threads deflate into their slots, the slots are written in order
  size_t K = nthreads > 1 ? (size_t)(nthreads > 64 ? 64 : nthreads) : 1;
  if (K > nblk) K = nblk;
  const size_t batch = K * 16 < nblk ? K * 16 : nblk;
  std::vector<uint8_t> slots(batch * kBlockMax);
  std::vector<size_t> sizes(batch);
  for (size_t b0 = 0; b0 < nblk; b0 += batch) {
    const size_t b1 = b0 + batch < nblk ? b0 + batch : nblk;
    std::atomic<size_t> next(b0);
    std::atomic<int> bad(0);
    auto work = [&]() {
      Deflater d;
      for (;;) {
        const size_t i = next.fetch_add(1);
        if (i >= b1) break;
        const size_t lo = i * kBlockIn, len = n - lo < kBlockIn ? n - lo : kBlockIn;
        sizes[i - b0] = make_block(d, data + lo, len, slots.data() + (i - b0) * kBlockMax);
        if (sizes[i - b0] == 0) bad = 1;
      }
    };
    std::vector<std::thread> th;
    const size_t nt = K < b1 - b0 ? K : b1 - b0;
    for (size_t t = 1; t < nt; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
    if (bad) return fail(EPI_ERR_STATE, "BGZF compression failed");
    for (size_t i = b0; i < b1; i++)
      if (fwrite(slots.data() + (i - b0) * kBlockMax, 1, sizes[i - b0], static_cast<FILE *>(f_)) != sizes[i - b0])
        return fail(EPI_ERR_ARG, "Unable to write BAM");
  }
  return EPI_OK;
}

int BgzfWriter::close() {
  static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (!f_) return fail(EPI_ERR_STATE, "BGZF writer is not open");
  FILE *f = static_cast<FILE *>(f_);
  f_ = nullptr;
  const bool ok = fwrite(eof, 1, sizeof(eof), f) == sizeof(eof);
  if (fclose(f) != 0 || !ok) return fail(EPI_ERR_ARG, "Unable to write BAM");
  return EPI_OK;
}

}  // namespace epi

extern "C" int epi_bgzf_write_file(const char *path, const uint8_t *data, int64_t n, int nthreads) {
  if (n < 0 || (n > 0 && !data)) return fail(EPI_ERR_ARG, "epi_bgzf_write_file: bad arguments");
  try {
    BgzfWriter w;
    EPI_TRY(w.open(path));
    EPI_TRY(w.write(data, (size_t)n, nthreads));
    return w.close();
  } catch (const std::bad_alloc &) {
    return fail(EPI_ERR_NOMEM, "epi_bgzf_write_file: out of host memory");
  }
}
