// Position-congruent row layout: the batch's own copy of xm in which row x starts at an offset congruent to its start
// position modulo A (16; 4 on request), i.e. behind up to A - 1 bytes of filler.
//
// Why: the tile kernels (cx_report.hip, mhl_fused.hip) request POSITION-aligned 16-byte chunks -- a dword of xm then maps
// onto one LDS cell of four positions -- at the address  xm + off[x] - (start[x] - tile position 0) + 16 c.  With rows
// back to back that address has any byte alignment, and a global_load_dwordx4 that is not dword-aligned runs at about
// 0.85 of the rate of an aligned one (scratch/align_cost.py on the product kernels: config-2 stream with every row
// aligned 0.72-0.74 ms, every row misaligned 0.83-0.90, the uniform mix 0.81; profiles/r04_layout.txt).  The reference
// keeps one std::string per template (src/epialleleR.h:28-38), so where a row starts in the arena is this engine's own
// business: off[x] = start[x] (mod 16) makes every chunk of every row 16-byte aligned at no cost per report.  The byte
// format of a row is untouched; the filler between rows is never interpreted (first / last chunk of a row are masked to
// the row's own bytes by every kernel).
//
// Cost: one pass at batch creation (read B bytes, write B + <= 15 n), 7.5 bytes per row on average (2.5 % for PE150
// templates), and int32 len[] next to off[] (rows no longer end where the next one starts).  epi_batch_upload does it
// as part of the upload; for an adopted batch (caller-owned device memory) it is the caller's choice: epi_batch_realign.
#include "common.hpp"
#include <utility>

namespace epi {

constexpr int LY_WG = 256, LY_ITEMS = 4;          // the offset scan: 1024 rows per workgroup

// what row x adds to the running offset: its bytes and the filler behind it, so that row x + 1 starts congruent to its
// start position (by induction: off[x] = start[x] (mod A) and off[x + 1] = off[x] + len + ((start[x + 1] - start[x] - len) mod A))
__device__ __forceinline__ uint32_t ly_item(const int32_t *__restrict__ start, const int32_t *__restrict__ len, int64_t x, int64_t n,
                                            uint32_t am) {
  const uint32_t l = (uint32_t)len[x];
  const uint32_t pad = x + 1 < n ? ((uint32_t)start[x + 1] - ((uint32_t)start[x] + l)) & am : 0u;
  return l + pad;
}

struct LyItem {                                    // element x of the offset scan
  const int32_t *start, *len;
  int64_t n;
  uint32_t am;
  __device__ unsigned long long operator()(int64_t x) const { return ly_item(start, len, x, n, am); }
};
struct LyStoreOffset {
  int64_t *off;
  __device__ void operator()(int64_t x, unsigned long long ex, unsigned long long) const { off[x] = (int64_t)ex; }
};

struct __attribute__((packed, aligned(1))) LyU4u { uint32_t x, y, z, w; };

// G lanes copy the part of a row that lies in source bytes [c0, c1) -- `src` holds exactly those bytes (the whole old arena:
// c0 = 0; a staged piece of an upload: src[0] is source byte c0) -- to its place in the new arena: the bytes up to the first
// 16-byte boundary of the destination and behind the last one singly, the chunks in between as aligned 16-byte stores (of
// 16-byte loads at the source's alignment).  The piece that holds the END of row x (c0 < end <= c1, or end = 0 in the first
// piece) also writes the filler between row x and row x + 1, so every byte between off[0] and off[n] is written exactly once.
template <int G>
__global__ __launch_bounds__(256) void k_ly_copy(const uint8_t *__restrict__ src, int64_t c0, int64_t c1, const int64_t *__restrict__ src_off,
                                                  const int32_t *__restrict__ len, const int64_t *__restrict__ dst_off, int64_t row_a,
                                                  int64_t nrows, uint8_t *__restrict__ dst) {
  const int sub = threadIdx.x & (G - 1);
  const int64_t k = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
  if (k >= nrows) return;
  const int64_t x = row_a + k;
  const int64_t s = src_off[x], d = dst_off[x];
  const int64_t L = len[x], e = s + L;
  int64_t lo = c0 > s ? c0 - s : 0, hi = (c1 < e ? c1 : e) - s;    // the row's bytes [lo, hi) are in this piece
  if (hi > lo) {
    const uint8_t *sp = src + (s - c0) + lo;
    uint8_t *dp = dst + d + lo;
    const int64_t nby = hi - lo;
    int64_t h = (16 - ((d + lo) & 15)) & 15;
    if (h > nby) h = nby;
    for (int64_t i = sub; i < h; i += G) dp[i] = sp[i];
    const int64_t nfull = (nby - h) >> 4;
    for (int64_t q = sub; q < nfull; q += G) {
      const LyU4u v = *reinterpret_cast<const LyU4u *>(sp + h + (q << 4));
      *reinterpret_cast<uint4 *>(dp + h + (q << 4)) = make_uint4(v.x, v.y, v.z, v.w);
    }
    for (int64_t i = h + (nfull << 4) + sub; i < nby; i += G) dp[i] = sp[i];
  }
  if ((e > c0 && e <= c1) || (e == 0 && c0 == 0)) {
    const int64_t gap = dst_off[x + 1] - d - L;                     // filler behind the row (0 .. 15)
    for (int64_t i = sub; i < gap; i += G) dst[d + L + i] = (uint8_t)0xFB;
  }
}

// lanes per row of the copy by the mean row (a long-read batch: a wavefront per row)
int layout_group(int64_t nbytes, int64_t n) {
  const int64_t mean = n > 0 ? nbytes / n : 0;
  int g = 8;
  while (g < 64 && (int64_t)g * 64 < mean) g <<= 1;
  return g;
}

int layout_copy_range(const uint8_t *src, int64_t c0, int64_t c1, const int64_t *src_off, const int32_t *len, const int64_t *dst_off,
                      int64_t row_a, int64_t nrows, int g, uint8_t *dst, hipStream_t s) {
  if (nrows <= 0) return EPI_OK;
  const unsigned blocks = (unsigned)((nrows * g + 255) / 256);
#define EPI_LY(GG) hipLaunchKernelGGL((k_ly_copy<GG>), dim3(blocks), dim3(256), 0, s, src, c0, c1, src_off, len, dst_off, row_a, nrows, dst)
  if (g == 8) EPI_LY(8); else if (g == 16) EPI_LY(16); else if (g == 32) EPI_LY(32); else EPI_LY(64);
#undef EPI_LY
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

// The congruent offsets of the batch's rows (from start[] and len[]) into new_off [n + 1]; *h_end = the end of the data,
// *head = the filler in front of row 0.  One host synchronisation (the arena is allocated to size).
int layout_offsets(epi_batch *b, int modulus, hipStream_t s, DevBuf *new_off, unsigned long long *h_end, uint32_t *head) {
  const int64_t n = b->n;
  const uint32_t am = (uint32_t)modulus - 1u;
  DevBuf tmp;
  EPI_TRY(new_off->ensure((size_t)(n + 1) * 8));
  int64_t *off = new_off->as<int64_t>();
  unsigned long long *d_end = reinterpret_cast<unsigned long long *>(off + n);   // the scan's total is off[n]
  int32_t first_start = 0;
  EPI_TRY(read_scalars(b, s, b->start, 4, &first_start));
  *head = (uint32_t)first_start & am;
  EPI_TRY((device_scan<SumU64, LY_ITEMS, LY_WG>(n, LyItem{b->start, b->len, n, am}, LyStoreOffset{off}, (unsigned long long)*head, d_end,
                                                tmp, s)));
  return read_scalars(b, s, d_end, 8, h_end);                // (synchronises: tmp may go)
}

int realign_batch(epi_batch *b, int modulus, hipStream_t s) {
  if (modulus != 4 && modulus != 8 && modulus != 16) return fail(EPI_ERR_ARG, "realign: modulus must be 4, 8 or 16");
  if (b->congruent == modulus || b->n == 0) { b->congruent = modulus; return EPI_OK; }
  if (!b->stats_queued || !b->len) return fail(EPI_ERR_STATE, "realign: the batch has no row lengths yet");
  if (b->last_kind != KIND_NONE) return fail(EPI_ERR_STATE, "epi_batch_realign: call it before the first report on the batch");
  EPI_HIP(hipStreamWaitEvent(s, b->stats_done, 0));       // len[] is written by k_row_stats, possibly on another stream
  DevBuf new_off, new_xm;
  unsigned long long h_end = 0; uint32_t head = 0;
  EPI_TRY(layout_offsets(b, modulus, s, &new_off, &h_end, &head));
  const size_t cap = ((size_t)h_end + 15) / 16 * 16 + 64;
  EPI_TRY(new_xm.ensure(cap));
  uint8_t *dst = new_xm.as<uint8_t>();
  if (head && hipMemsetAsync(dst, 0xFB, head, s) != hipSuccess) return fail(EPI_ERR_HIP, "realign: memset failed");
  if (hipMemsetAsync(dst + h_end, 0xFB, cap - (size_t)h_end, s) != hipSuccess) return fail(EPI_ERR_HIP, "realign: memset failed");
  EPI_TRY(layout_copy_range(b->xm, 0, INT64_MAX, b->off, b->len, new_off.as<int64_t>(), 0, b->n, layout_group(b->nbytes, b->n), dst, s));
  // The old arena may be handed back to its owner (an adopted batch) when this returns, or freed (an uploaded one): new_off / new_xm
  // hold the batch's previous buffers after the swaps below and free them on return.  This synchronisation makes that safe.
  if (hipStreamSynchronize(s) != hipSuccess) return fail(EPI_ERR_HIP, "realign: %s", hipGetErrorName(hipGetLastError()));
  if (!b->owns) {
    // an adopted batch: the three small columns become the batch's own as well -- from here on nobody else can change a
    // row, and what is derived from the rows alone (the tile table, tiles.hip) stays valid between reports
    const size_t cb = (size_t)b->n * 4;
    for (DevBuf *d : {&b->own_rname, &b->own_strand, &b->own_start}) EPI_TRY(d->ensure(cb + 4));
    if (hipMemcpyAsync(b->own_rname.p, b->rname, cb, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(b->own_strand.p, b->strand, cb, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipMemcpyAsync(b->own_start.p, b->start, cb, hipMemcpyDeviceToDevice, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) return fail(EPI_ERR_HIP, "realign: column copy failed");
    b->rname = b->own_rname.as<int32_t>();
    b->strand = b->own_strand.as<int32_t>();
    b->start = b->own_start.as<int32_t>();
    b->owns = true;
  }
  std::swap(b->own_xm, new_xm);
  std::swap(b->own_off, new_off);
  b->xm = b->own_xm.as<uint8_t>();
  b->off = b->own_off.as<int64_t>();
  b->nbytes = (int64_t)h_end;
  b->congruent = modulus;
  b->cols_owned = true;
  return EPI_OK;
}

}  // namespace epi

using namespace epi;

extern "C" int epi_batch_realign(epi_batch *b, void *stream) {
  if (!b) return fail(EPI_ERR_ARG, "epi_batch_realign: NULL batch");
  EPI_HIP(hipSetDevice(b->eng->device));
  const int m = options().realign;
  if (m == 0) return EPI_OK;                               // EPIHIP_REALIGN=0: rows stay where the caller put them
  return realign_batch(b, m, pick_stream(b, stream));
}

extern "C" int epi_batch_layout(const epi_batch *b) { return b ? b->congruent : -1; }

// the rows as the kernels read them (device pointers owned by the batch or its creator; valid until the batch is freed or realigned)
extern "C" int epi_batch_view(const epi_batch *b, const uint8_t **d_xm, const int64_t **d_off, const int32_t **d_len, int64_t *nbytes) {
  if (!b) return fail(EPI_ERR_ARG, "epi_batch_view: NULL batch");
  if (d_xm) *d_xm = b->xm;
  if (d_off) *d_off = b->off;
  if (d_len) *d_len = b->len;
  if (nbytes) *nbytes = b->nbytes;
  return EPI_OK;
}
