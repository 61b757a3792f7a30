// Internal declarations shared by the engine's translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <map>
#include <memory>
#include <vector>
#include "../../include/epihip.h"
#include "xm_codes.hpp"

namespace epi {

// ---- errors ---------------------------------------------------------------
void set_error(const char *fmt, ...);
int fail(int code, const char *fmt, ...);

#define EPI_HIP(expr)                                                              \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess)                                                          \
      return ::epi::fail(_e == hipErrorOutOfMemory ? EPI_ERR_NOMEM : EPI_ERR_HIP,  \
                         "%s failed: %s (%s:%d)", #expr, hipGetErrorName(_e), __FILE__, __LINE__); \
  } while (0)

#define EPI_TRY(expr) do { int _rc = (expr); if (_rc != EPI_OK) return _rc; } while (0)
constexpr int EPI_RETRY_POOL = -77;   // internal (never leaves the library): a deferred sharded report found its row pool too small

// ---- geometry ---------------------------------------------------------------
#ifndef EPI_CX_TILE
#define EPI_CX_TILE 1024
#endif
constexpr int kTile = EPI_CX_TILE;     // positions per CX tile (absolute grid)
constexpr int kMhlTile = 512;          // positions per lMHL tile (56 B of LDS counters per position and strand)
constexpr int kCxPlanes = 16;          // [strand 2][counter 8] u32 planes of kTile entries
constexpr int64_t kPosBias = 1LL << 31;// makes (start + bias) non-negative for any int32 start; multiple of every tile size

// counter slots inside one strand's 8 planes
enum { SLOT_DOT = 0, SLOT_OTHER = 1, SLOT_H = 2, SLOT_h = 3, SLOT_X = 4, SLOT_x = 5, SLOT_Z = 6, SLOT_z = 7, SLOT_SKIP = 8 };

struct Tile {            // one work item of the tile kernels
  int64_t pos0;          // first position of the tile
  int32_t rname;
  int32_t row_lo, row_hi;// candidate rows: same rname, start in (pos0 - Lmax, pos0 + kTile)
  int32_t slot;          // >=0: accumulate into shared slab slot instead of emitting
};

// The scalars the kernels of a report and the host exchange (epi_batch::misc holds one of these; report_scalars()).  The
// tile-index pass (tiles.hip) leaves the tile count and zeroes the counters of the report that follows; the report reads
// the block back at its synchronisation.  Kernels take `&sc->field`, the host copies into an instance of its own.
struct Scalars {
  uint32_t ntiles;         // [0] tiles the index pass counted (0xFFFFFFFF: a remembered count no longer holds)
  uint32_t cursor;         // [1] rows handed out of the pool's overflow region (may exceed its size) ...
                           //     ... or, CX direct mode (no pool): tiles whose row count differed from the kept one
  uint32_t rows;           // [2] output rows: the total of the scan over the tiles' row counts
  uint32_t heavy_count;    // [3] CX, two-kernel lMHL: ultra-deep tiles set aside ...
                           //     ... or, one-pass lMHL kernel: deep tiles it listed for the two-kernel path
  uint32_t deep_count;     // [4] CX: tiles the lean kernel hands to the general one
  uint32_t fold_cursor;    // [5] one-pass lMHL kernel: slab slots handed out for folded call counters
  uint32_t unused6[2];
  uint32_t heavy_max;      // [8] candidate rows of the largest heavy tile
  uint32_t unused9[3];
  uint32_t rec_max[2];     // [12-13] two-kernel lMHL pass 1: a 64-bit maximum over the reads' record counts
  uint32_t max_h;          // [14] ... and the longest stretch
  uint32_t pat_total;      // [15] extractPatterns: patterns found
};
static_assert(offsetof(Scalars, ntiles) == 0 && offsetof(Scalars, cursor) == 4 && offsetof(Scalars, rows) == 8 &&
              offsetof(Scalars, heavy_count) == 12 && offsetof(Scalars, deep_count) == 16 && offsetof(Scalars, fold_cursor) == 20 &&
              offsetof(Scalars, heavy_max) == 32 && offsetof(Scalars, rec_max) == 48 && offsetof(Scalars, max_h) == 56 &&
              offsetof(Scalars, pat_total) == 60 && sizeof(Scalars) == 64, "Scalars layout");

// ---- device buffers that grow on demand --------------------------------------
// A DevBuf owns its allocation: move-only, freed by its destructor (engine.hip; release() frees early).  The device of
// the allocation must be current when it goes.  view() is the non-owning form -- a piece of somebody else's allocation
// for a callee that takes a DevBuf: never freed, never counted, and ensure() beyond its size is an error.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete; DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept { *this = static_cast<DevBuf &&>(o); }
  DevBuf &operator=(DevBuf &&o) noexcept {                    // the moved-from buffer is left empty
    if (this != &o) { release(); p = o.p; cap = o.cap; owned = o.owned; o.p = nullptr; o.cap = 0; o.owned = true; }
    return *this;
  }
  ~DevBuf();
  static DevBuf view(void *p, size_t bytes) { DevBuf v; v.p = p; v.cap = bytes; v.owned = false; return v; }
  int ensure(size_t bytes);   // keeps contents only if no growth is needed
  void release();
  template <class T> T *as() const { return reinterpret_cast<T *>(p); }
 private:
  bool owned = true;
};

// The scratch of a stateless call as one allocation, released when the call returns: a unit's layout reserves its pieces (which
// fixes `used`, the figure its *_scratch_bytes entry point states), alloc() takes the bytes, at() hands a piece out.  Pieces lie back
// to back in the order reserved, nothing padded in between: a layout puts 64-bit members first, and at() refuses a misaligned piece.
struct ScratchArena {
  DevBuf mem;
  size_t used = 0;
  // `bytes` at the current end; the piece takes up `bytes` rounded up to a multiple of `round` (a power of two)
  size_t reserve(size_t bytes, size_t round = 1) { const size_t at = used; used += (bytes + round - 1) & ~(round - 1); return at; }
  int alloc() { return mem.ensure(used); }
  template <class T> int at(size_t off, T **piece, size_t align = alignof(T)) const {   // align: where the kernels read wider than T
    if (off % align != 0) return fail(EPI_ERR_STATE, "scratch piece at byte %zu, not a multiple of the %zu its elements need", off, align);
    *piece = reinterpret_cast<T *>(mem.as<char>() + off);
    return EPI_OK;
  }
};

struct ProfEntry { double ms = 0; int64_t n = 0; };

// ---- state of the reports that count over the per-strand site table -------------
// The scalars their kernels and the host exchange (SiteReportState::scal holds one, 64 bytes allocated; kernels take
// `&sc->field`, as with Scalars)
struct SiteScalars {
  uint32_t nplus;          // '+' sites of the table: its '-' part starts here
  uint32_t nrow;           // reported rows: windows, pairs
  uint32_t nblock;         // haplotype blocks
  uint32_t ncommon;        // comparison: sites both batches have
  uint32_t nwords;         // FDRP: 64-bit words of the rows' packed calls
  uint32_t unused;
  unsigned long long ncalls;   // FDRP: calls of the kept rows = (site, row) pairs of the index (zeroed by the report)
};
static_assert(sizeof(SiteScalars) == 32 && offsetof(SiteScalars, ncalls) == 24, "SiteScalars layout");

// What the heterogeneity report (heterogeneity.hip), the linkage report and its blocks (linkage.hip), the heterogeneity
// comparison (het_compare.hip, on its first batch) and the FDRP report (fdrp.hip) keep on a batch, by owner: the site table
// (site_table.hpp has its construction and the data path), the workspace over it that each of them reuses, and per report
// what only its own fetch reads.  One of them is live on a batch at a time (last_kind).
struct SiteReportState {
  // the table (site_table.hip)
  DevBuf cx;               // in CX row order: the un-thresholded CX report's six columns, [6][nsite]
  DevBuf rank;             // [nsite] '+' rows in front of a CX row
  DevBuf key, sctx;        // [nsite] the table split per strand: 64-bit search key and context code of a site
  DevBuf scal;             // SiteScalars
  int64_t nsite = 0;       // sites of the table the last report counted over (0: it reported nothing, no table is kept)
  SiteScalars *scalars() const { return scal.as<SiteScalars>(); }
  // the workspace every report reuses
  DevBuf counts;           // [nsite][2^k] pattern counters, [nsite][D][4] pair counters, or FDRP's [nsite] FdrpSite
  DevBuf flag, out;        // keep flag and output row: [nsite] per window start or site, [nsite][D] per pair
  uint32_t min_reads = 1;  // the last report's floor: each report writes its own and its keep kernel and fetch read it back
  struct Het { int32_t k = 0; int64_t max_span = 0; } het;   // heterogeneity report and the comparison's windows: their size, the span cap
  struct Link {            // linkage report and its blocks
    int32_t D = 0; int64_t max_dist = 0;   // neighbours, the distance cap
    bool blocks = false;   // epi_batch_linkage_blocks_dev has run on the last linkage report ...
    int64_t nblock = 0;    // ... and found this many
    DevBuf back, blen, bmean;     // blocks, by table ordinal: leading linked pairs behind a site; length and mean r^2 at a block's first site
    DevBuf bflag, bout;           // ... by CX row: a block starts here, its output row
  } link;
  struct Cmp { DevBuf cx_all, counts_b; } cmp;   // comparison: a's CX table before the common one is compacted from it; the counters of b's rows
  struct Fdrp {            // FDRP report: the site -> rows index and the rows' packed calls
    int32_t W = 0, max_rows = 0, min_overlap = 0;   // flanking sites, rows used per site, overlap a pair needs
    DevBuf frow;           // [6][n rows] u32: first site, sites, calls and words of a row; its first pair and first word (scans)
    DevBuf fbits;          // [2][nwords] u64: the rows' calls, bit j of a row = its site lo + j: valid, then methylated
    DevBuf fpair;          // the (site, row) pairs and the sort's scratch; sorted: rows of site g at [site_off[g], site_end[g])
    DevBuf fsite;          // [2][nsite] u32 site_off, site_end
  } fdrp;
};

// ---- per-read class counting shared by the per-read kernels and the fused CX tile kernel (per_read.hip) ----------
// (ClassLut, the table the class strings become: xm_codes.hpp)
struct ThrParams {                                   // rcpp_threshold_reads.cpp:15-23
  uint32_t min_n_ctx;
  double min_ctx_meth_frac, max_ooctx_meth_frac;
};
// 2-bit membership fields of up to four class strings in one LUT; false when a class string repeats a letter
bool make_field_lut(const char *const cls[4], ClassLut *out);

}  // namespace epi

struct epi_engine {
  int device = 0;
  hipStream_t stream = nullptr;       // default compute stream
  hipStream_t copy_stream = nullptr;  // H2D staging stream
  void *pinned[2] = {nullptr, nullptr};
  size_t pinned_bytes = 0;
  hipEvent_t pinned_done[2] = {nullptr, nullptr};
  // epi_batch_upload lays the rows out while they arrive (engine.hip, layout.hip): two device-side pieces of the source
  // arena, filled by the copy stream and emptied into the batch's own arena by kernels on aux_stream
  hipStream_t aux_stream = nullptr;
  void *dev_stage[2] = {nullptr, nullptr};
  size_t dev_stage_bytes = 0;
  hipEvent_t up_done[2] = {nullptr, nullptr}, stage_free[2] = {nullptr, nullptr};
  int32_t *h_scalars = nullptr;       // pinned scratch for small D2H reads (64 x int64)
};

namespace epi {
struct RowStats {          // filled by k_row_stats
  int32_t max_len;
  int32_t unsorted;        // !=0: some row violates (rname,start) order
  int32_t bad_strand;      // !=0: strand not in {1,2}
  int32_t bad_len;         // !=0: off not non-decreasing
  int32_t deep;            // !=0: some position may be covered by more than 255 rows (row x + 255 starts inside row x)
  // rows by the number of position-aligned 16-byte chunks a row can span, (len + 30) / 16: bin k counts the rows with at most
  // kLenBins[k] chunks that did not fit bin k - 1 (the last bin: everything longer).  The tile kernels pick their lane shape
  // from this, not from the longest row (one 1 kb template among 100 000 PE150 ones must not widen the shape for all).
  uint32_t len_hist[14];
};
constexpr int kLenBinCount = 14;
constexpr int kLenBins[kLenBinCount] = {12, 16, 20, 24, 32, 40, 48, 64, 80, 96, 128, 160, 192, 0x7FFFFFFF};
}  // namespace epi

struct epi_shard_plan;      // comm.hip: shared tile keys of a (batch, tile grid, communicator) triple

namespace epi {
// What the last report call left on a batch; the first half of a sharded report is continued by its *_finish_shared call
enum ReportKind {
  KIND_NONE = 0,
  KIND_CX = 1,              // finished CX report
  KIND_MHL = 2,             // finished lMHL report
  KIND_CX_SHARED = 3,       // first half of a sharded CX report
  KIND_MHL_SHARED = 4,      // ... of a sharded lMHL report, two-kernel path (slabs in k_mhl_tiles' layout)
  KIND_MHLF_SHARED = 5,     // ... of a sharded lMHL report, one-pass kernel (slabs in its layout, mhl_common.hpp)
  KIND_HET = 6,             // finished heterogeneity report
  KIND_LINK = 7,            // finished linkage report
  KIND_HETCMP = 8,          // finished heterogeneity comparison (on its first batch; the second is left at KIND_NONE)
  KIND_FDRP = 9,            // finished FDRP report
};

// ---- what a batch keeps besides its rows, one struct per owner (who owns a device buffer) ----------------------
// The tile index (tiles.hip).  The tile table is a function of (rname, start, longest row, tile size, shared keys): while the
// batch owns its columns the table of the last build is still valid for the same tile size and keys, and build_tiles skips the pass.
struct TileIndex {
  DevBuf tiles, nt_dev;                         // nt_dev: the tile count as the index pass left it in Scalars::ntiles
  struct { int32_t T = 0, nt = 0, lmax = 0; std::vector<int64_t> shared; } built;   // what `tiles` was built for (T = 0: nothing)
  // tile counts of this (immutable) batch by tile size, as found by earlier calls, and the index build's scanned per-block counts
  struct { int32_t T = 0, nt = 0, lmax = 0; DevBuf bsum; } hint[4];
  void forget() { for (auto &h : hint) h.T = 0; built.T = 0; }   // the rows changed: nothing remembered holds any more
};

// Row pool of a report: a slot per tile + an overflow region (the scheme: tiles.hip, with layout_pool).  Each report's
// bind function names what it keeps in a .. f.
struct RowPool {
  DevBuf tile_nrow, tile_base, tile_out;
  DevBuf key, a, b, c, d, e, f;
  size_t row_cap = 0, row_cap2 = 0;             // rows that fit key / a / b; rows that fit d / e (lMHL doubles)
  DevBuf heavy_list, heavy_slab, heavy_sums;    // ultra-deep tiles: ids and dense counters (+ lMHL sums)
};

struct CxState {                                // cx_report.hip
  uint32_t slot_cg = 0, slot_wide = 0;          // pool rows per tile slot: CpG-only reports / reports with CHG, CHH (adapted per call)
  uint32_t last_slot = 0, last_ovf = 0;         // layout of the last CX report (the sharded second half emits into it)
  int last_np = 0; uint32_t last_ctx_of_plane = 0;   // ... its number of reported contexts and their codes
  // CX reports written straight into the caller's columns (direct mode): the tile offsets and row counts of the last
  // pool report, for its context mask (key = mask | 1 << 31; 0: none), tile size and tile count
  struct { DevBuf off, cnt; uint32_t key = 0; int32_t T = 0, nt = 0; int64_t nrow = 0; } kept;
  // One host synchronisation for a sharded CX report (comm.hip asks for it: cx_report_shared's `defer`): the first half
  // queues its kernels and returns without reading anything back (`deferred`); the second half reads and checks everything
  // at once.  Allowed only when an earlier report on this (immutable) batch and tile size found no ultra-deep tile that the
  // host would have to finish before the slab may travel (noheavy_T / _rows: the tile size and threshold that was observed for).
  bool deferred = false; uint32_t def_heavy_done = 0; int32_t noheavy_T = 0, noheavy_rows = 0;
  DevBuf deep_list;                             // tiles the lean kernel hands to the general one
  DevBuf pass_tmp;                              // pass flags when thresholding could not be fused and the caller wants none
  DevBuf thr_tab;                               // fused thresholding: decision table for thr_tab_prm over totals 0..thr_tab_len
  int32_t thr_tab_len = -1; ThrParams thr_tab_prm = {0, 0.0, 0.0};
};

struct MhlState {                               // mhl_report.hip, mhl_fused.hip
  DevBuf m, h, blk, cont, cur;                  // pass 1: stretch records, per-read info, record table, block carries
  size_t rec_cap = 0;                           // records that fit m
  uint32_t slot = 0, last_slot = 0, last_ovf = 0, ctx_mask = 0;   // pool rows per tile slot and the last report's layout, as for CX; its contexts
  DevBuf keep_tab;                              // fused lMHL: passing out-of-context counts per total (k_mhl_keep_table)
  int32_t keep_len = -1; double keep_oo = 0.0;
  uint32_t fused_slot = 0;                      // `slot` of the fused kernel (1024-position tiles)
  bool prefer_wide = false;                     // most tiles of the last fused lMHL report needed the u64 sums: start with that variant
  uint32_t prefer_wide_H = 0;                   // ... learned for this haplotype clamp H (the sums shrink with H: a smaller one probes the fast variant again)
  bool prefer_fold = false;                     // ... many held more than 255 rows: use the kernel with the folded call counters
  DevBuf fold_slab;                             // call counters of tiles over 255 rows (kernels built without the LDS fold array)
};

// multi-GPU shared tiles (comm.hip): which tiles dump their raw sums into a slab, and the slab(s) attached for them
enum SlabKind { SLAB_NONE, SLAB_CX, SLAB_MHL, SLAB_MHL_FUSED };   // _MHL: k_mhl_tiles' layout; _MHL_FUSED: the fused kernel's (mhl_common.hpp)
// Elements of the slabs per shared tile, int32 counters and int64 sums (none for CX): the one place besides the kernels that
// knows them (tiles.hip).  T: the CX report's tile size (it depends on the contexts reported; each lMHL kernel has its own).
struct SlabShape { size_t cnt, sum; };
SlabShape slab_shape(SlabKind kind, int T);
struct ShardState {
  std::vector<int64_t> keys, dev_keys;          // dev_*: what d_keys / d_owned currently hold
  std::vector<int32_t> owned, dev_owned;
  DevBuf d_keys, d_owned, d_slot_tile;
  SlabKind kind = SLAB_NONE;                    // what is attached (attach_shared), in the caller's memory or the two buffers below:
  int32_t *d_cnt = nullptr;                     // ... the counter slab
  int64_t *d_sum = nullptr;                     // ... the sum slab (none for SLAB_CX)
  // the library's own sharded entry points (comm.hip): their slabs and the plans they remember.  A CX report has no sums:
  // lib_sum then serves as the scratch counter slab of its pool retry.
  DevBuf lib_cnt, lib_sum;
  std::vector<std::shared_ptr<epi_shard_plan>> plans;
};

// The pair table of the last allele-specific methylation report (asm_report.hip): one piece per group of sites, in site
// order.  Nothing else on the batch reads or writes it; it goes with the batch.
struct AsmState {
  std::vector<DevBuf> piece;                    // [10][rows] int32: the pair rows' integer columns
  std::vector<int64_t> rows;                    // rows of every piece
  int64_t npair = 0;
  bool reported = false;                        // a report has run: a fetch has a table (possibly empty) to write
  void clear() { piece.clear(); rows.clear(); npair = 0; reported = false; }
};

struct PatternStats {
  int64_t extract_groups = 0, extract_pairs = 0, extract_scratch = 0;        // last epi_batch_extract_patterns_multi: groups, pairs, peak scratch bytes
  int64_t summarise_groups = 0, summarise_pairs = 0, summarise_fallback = 0; // last epi_batch_summarise_patterns_multi: groups, pairs, targets grouped on the host
};
}  // namespace epi

struct epi_batch {
  epi_engine *eng = nullptr;
  int64_t n = 0, nbytes = 0;
  // Rows as every kernel sees them: row x owns xm[off[x] .. off[x] + len[x]); off has n + 1 non-decreasing entries
  // (off[n] = end of the data = nbytes), rows do not overlap, gaps between them are allowed.  The constructors take rows
  // back to back (include/epihip.h) and fill `len` from the offsets; epi_batch_realign (layout.hip) replaces xm / off by
  // the batch's own POSITION-CONGRUENT copy: off[x] = start[x] (mod 16), so that the position-aligned 16-byte chunks the
  // tile kernels request are address-aligned (byte-misaligned dwordx4 loads run at ~0.85 of the rate).
  const uint8_t *xm = nullptr;
  const int64_t *off = nullptr;
  const int32_t *len = nullptr;
  const int32_t *rname = nullptr, *strand = nullptr, *start = nullptr;
  bool owns = false;
  int congruent = 0;         // 0: rows as the caller laid them out; 4 / 16: off[x] = start[x] modulo this
  bool cols_owned = false;   // every column is the batch's own copy (uploaded, or adopted and realigned): nobody can change a row
  epi::DevBuf own_xm, own_off, own_len, own_rname, own_strand, own_start;
  epi::DevBuf stats;        // RowStats of the batch (k_row_stats, queued once at creation)
  bool stats_queued = false, stats_host = false;
  hipEvent_t stats_done = nullptr;          // recorded behind k_row_stats on the stream it was queued on
  epi::RowStats h_stats = {};   // host copy, fetched by the first report call (which raises the errors)

  epi::TileIndex tix;
  epi::RowPool pool;
  epi::CxState cx;
  epi::MhlState mhl;
  epi::ShardState shard;
  epi::PatternStats pat;
  epi::AsmState asmr;
  // the heterogeneity report, the linkage report with its blocks, the heterogeneity comparison and the FDRP report: the
  // site table they count over (site_table.hpp) and what the last of them left for its fetch
  epi::SiteReportState sites;

  // workspace every report shares
  epi::DevBuf scan_tmp;
  epi::DevBuf misc;         // epi::Scalars (256 bytes allocated)
  epi::DevBuf diag;         // check / timing builds only
  epi::DevBuf host_io;      // device side of the host-pointer calls (pass flags / per-read beta)
  epi::DevBuf bf_flag;      // base frequencies: the sites' sortedness verdict (base_freqs.hip)

  // state of the last report (for fetch)
  epi::ReportKind last_kind = epi::KIND_NONE;
  int64_t last_nrow = 0;
  int32_t last_ntiles = 0;
};

// Somebody else may have changed the rows of this batch (a tile count remembered for it no longer holds): forget
// everything that was derived from row contents.
inline void batch_rows_changed(epi_batch *b) {
  b->tix.forget();
  b->cx.kept.key = 0;
  b->cx.noheavy_T = 0;
}

namespace epi {

hipStream_t pick_stream(epi_batch *b, void *stream);
// device -> host memory of the caller, complete on return.  Page-locked destinations are written by the DMA engine
// directly; pageable ones (malloc, R vectors) go through the engine's two pinned staging buffers in chunks, the copy
// out of buffer k overlapping the DMA into buffer k + 1.  `parts` may list several (dst, src, bytes) pieces: one pipeline.
struct CopyPart { void *dst; const void *src; size_t bytes; };
int copy_parts_to_host(epi_engine *eng, const CopyPart *parts, int nparts, hipStream_t s);
int copy_to_host(epi_engine *eng, void *h_dst, const void *d_src, size_t bytes, hipStream_t s);
int read_scalars(epi_engine *e, hipStream_t s, const void *d_src, size_t bytes, void *h_dst);  // sync D2H of a few bytes
int read_scalars(epi_batch *b, hipStream_t s, const void *d_src, size_t bytes, void *h_dst);   // ... on the batch's engine
inline Scalars *report_scalars(const epi_batch *b) { return b->misc.as<Scalars>(); }
inline int read_report_scalars(epi_batch *b, hipStream_t s, Scalars *h) {                   // the whole block, one sync
  return read_scalars(b, s, report_scalars(b), sizeof(Scalars), h);
}

// Host blocks of library-owned report tables (capi.hip).  A large block given back by epi_*_table_free is kept (two blocks,
// at most 1 GiB) and handed to the next table of a similar size: its pages are already mapped, where a fresh 168 MB block
// costs ~9 ms of page faults on the copy threads -- twice the copy itself.
void *table_block(size_t bytes);
void table_block_release(void *p);

// The bytes of a plain, gzip or BGZF file (bam_pack.cpp: BGZF blocks inflated by `nthreads` threads).
int read_text_file(const char *path, std::vector<uint8_t> &out, int nthreads);

// BGZF output (bgzf_writer.cpp): blocks of at most 0xff00 input bytes, deflated by `nthreads` threads, written in order;
// close() appends the end-of-file block.  Each write() ends with a short block (callers write large pieces).
class BgzfWriter {
 public:
  BgzfWriter() = default;
  BgzfWriter(const BgzfWriter &) = delete;
  BgzfWriter &operator=(const BgzfWriter &) = delete;
  ~BgzfWriter();
  int open(const char *path);
  int write(const uint8_t *data, size_t n, int nthreads);
  int close();
 private:
  void *f_ = nullptr;
};

// genome.cpp: the genome's bytes and contig offsets on `device`, uploaded by the first call there and kept resident
int genome_device(epi_genome *g, int device, const uint8_t **d_seq, const int64_t **d_off);

// call_methylation.hip: one window of records to call.  The host fills the records and the packed CIGAR / SEQ arrays
// while it parses the BAM records; the kernels write each record's l_seq output bytes to xm + xm_off, in one of two
// forms: the XM letters (callMethylation) or the packed template bytes (nt16 << 4) | ctx_to_idx(XM) (preprocessBam
// with a genome).
enum CallForm { CALL_XM = 0, CALL_PACKED = 1 };
struct CallRec {
  int64_t cig_off;     // first CIGAR op in the window's packed u32 array
  int64_t seq_off;     // first byte of the record's 4-bit SEQ in the window's packed array
  int64_t xm_off;      // first XM byte of the record in the window's output
  int32_t tid, pos;    // contig (genome index) and 0-based leftmost position
  int32_t l_seq, n_cig;
  uint8_t s_meth, s_conv;   // the strand tag's two characters: 'C','T' (forward table) or 'G','A' (reverse table)
  uint8_t pad[6];
};
static_assert(sizeof(CallRec) == 48, "CallRec layout");
struct CallWork { DevBuf recs, cig, seq, ref, xm; };   // device buffers of the windows, grown on demand
int call_methylation_window(epi_engine *eng, epi_genome *g, CallWork &wk, const CallRec *recs, int64_t nrec,
                            const uint32_t *cigar, int64_t ncig, const uint8_t *seq, int64_t nseq, int64_t nxm,
                            CallForm form, uint8_t *xm_out);

// assemble_templates.hip: preprocessBam(mates = "anywhere").  The reader uploads every kept record's CIGAR ops, packed
// query bytes (nt16 << 4) | ctx and QUAL to a device arena (at AsmRec::arena_off: 4 * n_cig bytes of ops, l_seq packed
// bytes, l_seq qualities); at the end of the file it knows each template's records in merge order and its output row,
// and the kernel merges them there.
struct AsmRec {
  int64_t arena_off;   // 4-byte aligned
  int32_t dest0;       // reference offset of the record's first aligned base from the template's start
  int32_t n_cig, l_seq;
  int32_t pad;
};
static_assert(sizeof(AsmRec) == 24, "AsmRec layout");
struct AsmTpl {
  int64_t out_off;     // the row's first byte in the output
  int64_t rec_lo;      // its records: AsmRec [rec_lo, rec_lo + nrec), in merge order
  int64_t q_off;       // rows wider than kAsmLdsWidth: their qualities in the global scratch (else unused)
  int32_t nrec;
  int32_t keep;        // row length: the template's width less both trims (0 when the trims cover it)
};
static_assert(sizeof(AsmTpl) == 32, "AsmTpl layout");
// Rows longer than this are merged in global memory (the row itself and a quality scratch) instead of LDS.
constexpr int kAsmLdsWidth = 2048;
// rows [0, ntpl) -> nbytes bytes at h_out (pinned or pageable); qbytes: the scratch the wide rows need.  The arena must
// be complete (the caller has synchronised its uploads).  *t_kernel, *t_d2h: seconds spent (synchronised).
int assemble_templates(epi_engine *eng, const uint8_t *d_arena, const AsmTpl *tpl, int64_t ntpl, const AsmRec *recs,
                       int64_t nrec, uint8_t q0, int32_t trim5, int64_t nbytes, int64_t qbytes, uint8_t *h_out,
                       double *t_kernel, double *t_d2h);
// The engine's two pinned staging buffers (engine.hip), for a producer that writes its bytes straight into them:
// stage_buffer waits until buffer k (0 or 1) is free and returns it; stage_send queues its first `bytes` to d_dst on
// the engine's copy stream.  The caller synchronises the copy stream after its last send.
int stage_buffer(epi_engine *eng, int k, uint8_t **buf, size_t *cap);
int stage_send(epi_engine *eng, int k, void *d_dst, size_t bytes);

// util kernels (util.hip)
int scan_exclusive_u32(const uint32_t *d_in, uint32_t *d_out, int64_t n, uint32_t *d_total,
                       DevBuf &tmp, hipStream_t s);
inline size_t scan_tmp_bytes(int64_t n) { return (size_t)((n + 4095) / 4096 * 4); }   // what it takes of tmp: its block sums
int scan_block_sums_inplace(uint32_t *d_bsum, int64_t nb, uint32_t *d_total, hipStream_t s);

// tile index (tiles.hip)
// queue k_row_stats for a new batch (no sync, no error: per-read functions accept unsorted rows)
int launch_row_stats(epi_batch *b, hipStream_t s);
// host copy of the statistics (waits for the kernel whatever stream it was queued on); no validation
int fetch_row_stats(epi_batch *b, hipStream_t s);
// layout.hip: the batch's own position-congruent copy of xm (see epi_batch); `modulus` 4 or 16
int realign_batch(epi_batch *b, int modulus, hipStream_t s);
int layout_offsets(epi_batch *b, int modulus, hipStream_t s, DevBuf *new_off, unsigned long long *h_end, uint32_t *head);
int layout_group(int64_t nbytes, int64_t n);
// rows [row_a, row_a + nrows): their bytes inside source bytes [c0, c1) (src[0] = source byte c0) to their place in dst
int layout_copy_range(const uint8_t *src, int64_t c0, int64_t c1, const int64_t *src_off, const int32_t *len, const int64_t *dst_off,
                      int64_t row_a, int64_t nrows, int g, uint8_t *dst, hipStream_t s);
// row statistics (validated: errors for bad offsets/strands/unsorted rows) + tile table; one host sync
// `hinted` (may be null): the caller accepts a tile count remembered from an earlier call on this batch and tile size
// (no host round trip in the middle of the index build) and verifies it against Scalars::ntiles at its own synchronisation.
int build_tiles(epi_batch *b, hipStream_t s, int32_t tile_positions, RowStats *h_stats, int32_t *ntiles_out, bool *hinted = nullptr);
// What every *_set_shared entry point does behind its argument checks (tiles.hip): the shared tile keys, which of them this
// rank owns, and the slabs of `kind` their tiles add into; nshared = 0 detaches everything.
int attach_shared(epi_batch *b, const int64_t *h_keys, const int32_t *h_owned, int32_t nshared, SlabKind kind, int32_t *d_cnt, int64_t *d_sum);
// Zeroes the attached slabs behind what `s` holds: a rerun of a first half adds into them again.  T: as for slab_shape.
int zero_shared_slabs(epi_batch *b, int T, hipStream_t s);
// Tail of every sharded report's second half, behind its owners' emit (tiles.hip): the tiles' row offsets, the one
// synchronisation, `deferred` (may be null: checks the first half left for this read-back), the pool check against the
// report's overflow base and capacity, the finished report's state (`done`).
int finish_shared_rows(epi_batch *b, hipStream_t s, ReportKind done, size_t ovf_base, size_t pool_cap, const char *overflow_msg,
                       int (*deferred)(epi_batch *, const Scalars &), int64_t *nrow_out);

// First half of the library's sharded CX report (cx_report.hip): epi_batch_cx_report_dev (thr = null) or
// epi_batch_cytosine_report_dev, which never defer; defer: where the batch allows it, read nothing back (CxState::deferred).
struct CxThreshold {                      // fused thresholding request (null = use the pass vector)
  const char *cls[4];
  ThrParams prm;
  static CxThreshold of(const char *ctx_meth, const char *ctx_unmeth, const char *ooctx_meth, const char *ooctx_unmeth, uint32_t min_n_ctx,
                        double min_ctx_meth_frac, double max_ooctx_meth_frac) {
    return {{ctx_meth, ctx_unmeth, ooctx_meth ? ooctx_meth : "", ooctx_unmeth ? ooctx_unmeth : ""}, {min_n_ctx, min_ctx_meth_frac, max_ooctx_meth_frac}};
  }
};
int cx_report_shared(epi_batch *b, const int32_t *d_pass, const CxThreshold *thr, int32_t *d_pass_out, const char *ctx, bool defer,
                     hipStream_t s, int64_t *nrow_out);

// Row pool of a report: a slot per tile + an overflow region (the scheme: tiles.hip, with layout_pool)
struct PoolLayout {
  uint32_t slot;            // pool rows per tile slot (0: every tile through the cursor)
  size_t ovf_base;          // first row of the overflow region = nt * slot
};
int layout_pool(epi_batch *b, uint32_t slot, int T, int32_t nt, size_t headroom, int hook_slot, int (*reserve)(epi_batch *, size_t rows),
                PoolLayout *out);

// Result-neutral switches (test hooks that steer a call onto a rarely taken path, A/B shapes): read from the environment
// ONCE per process into this struct; epi_options_reload() re-reads it (tests that change a hook inside one process).
struct Options {
  int device = 0;            // EPIHIP_DEVICE        device of the default engine (host-pointer entry points)
  int cx_slot = -1;          // EPIHIP_CX_SLOT       pool rows per tile slot of the CX report (-1: adaptive)
  int cx_lean = 1;           // EPIHIP_CX_LEAN=0     the general (u16-folding) CX kernel for every tile
  int cx_direct = 1;         // EPIHIP_CX_DIRECT=0   CX reports through the row pool and the gather even where the tile kernel could
                             //                      write the caller's columns
  int heavy_rows = 0;        // EPIHIP_HEAVY_ROWS    candidate rows above which a tile is split / set aside (0: default)
  int tile_hint = 1;         // EPIHIP_TILE_HINT=0   tile index counted and scanned by every call
  int realign = 16;          // EPIHIP_REALIGN=0/4/8/16 epi_batch_upload / epi_batch_realign: keep the rows back to back / start them at
                             //                      offsets congruent to their start position modulo 4 / 16 (layout.hip)
  int mhl_fused = 1;         // EPIHIP_MHL_FUSED=0   two-kernel lMHL path for every batch
  int mhl_slot = -1;         // EPIHIP_MHL_SLOT
  int mhl_wg = 0;            // EPIHIP_MHL_WG        256 / 512 (two-kernel path)
  int mhl_tile_group = 0;    // EPIHIP_MHL_TILE_GROUP
  int mhl_multi = 0;         // EPIHIP_MHL_MULTI     wavefront-per-read pass 1
  int mhl_sums = 0;          // EPIHIP_MHL_SUMS      32 / 64
  int mhlf_fold = -1;        // EPIHIP_MHLF_FOLD=0/1 one-pass lMHL kernel without / with the LDS array of folded call counters (-1: by the batch)
  int mhlf_fold_slots = -1;  // EPIHIP_MHLF_FOLD_SLOTS  slab slots of the kernel without it (-1: default)
  int pr_group = 0;          // EPIHIP_GROUP         lanes per read of the general per-read kernel
  int pr_rpg = 0;            // EPIHIP_PR_RPG
  int pr_wide = 1;           // EPIHIP_PR_WIDE=0
  int bam_timing = 0;        // EPIHIP_BAM_TIMING    phase times of the BAM reader and of callMethylation on stderr
  int no_hugepage = 0;       // EPIHIP_NO_HUGEPAGE   plain malloc for the BAM reader's large buffers (A/B runs)
  int no_libdeflate = 0;     // EPIHIP_NO_LIBDEFLATE zlib's inflate for the BGZF blocks although libdeflate.so.0 can be loaded
  int pat_hash_bits = 0;         // EPIHIP_PAT_HASH_BITS=<k>  epi_batch_summarise_patterns_multi groups by the low k bits of the hash (1-63; else all 64)
  int64_t pat_group_bytes = 0;   // EPIHIP_PAT_GROUP_BYTES=<bytes>  scratch cap of a group of targets in epi_batch_extract_patterns_multi (0: 256 MiB)
  int64_t rgn_group_bytes = 0;   // EPIHIP_RGN_GROUP_BYTES=<bytes>  counter cap of a group of regions in epi_batch_region_report_dev (0: 256 MiB)
  int64_t asm_group_bytes = 0;   // EPIHIP_ASM_GROUP_BYTES=<bytes>  event cap of a group of sites in epi_batch_asm_report_dev (0: 256 MiB)
  int64_t upload_piece = 0; // EPIHIP_UPLOAD_PIECE=<bytes>  piece size of the host-to-device copies of epi_batch_upload (0: by the
                             //                      source; at most 64 MiB from pageable memory, the size of the pinned staging buffers)
};
const Options &options();

// profiling
void prof_begin(const char *name, hipStream_t s);
void prof_end(const char *name, hipStream_t s);

// Check build (`make check`: -DEPI_CHECK -DEPI_MHL_CHECK -> libepihip_check.so): the tile kernels verify the global
// addresses and pool indices they are about to use and record the first violation {code, v0, v1, block, thread}
// instead of performing the access; the host turns it into EPI_ERR_STATE.  Compiled out of the product library.
#ifdef __HIPCC__
#ifdef EPI_CHECK
__device__ __forceinline__ bool epi_dev_check(uint32_t *dbg, bool ok, uint32_t code, int64_t v0, int64_t v1) {
  if (!ok && dbg && atomicCAS(dbg, 0u, code) == 0u) {
    dbg[1] = (uint32_t)v0; dbg[2] = (uint32_t)v1; dbg[3] = blockIdx.x; dbg[4] = threadIdx.x; dbg[5] = (uint32_t)(v0 >> 32);
  }
  return ok;
}
#define EPI_DEV_CHECK(dbg, ok, code, v0, v1) epi_dev_check(dbg, ok, code, v0, v1)
#else
#define EPI_DEV_CHECK(dbg, ok, code, v0, v1) true
#endif
#endif

// Counter-based hashing (splitmix64's finaliser), shared by the synthetic generator (synth.hip) and simulateBam's random
// bases (simulate_bam.hip); tests/synth_np.py and epialleler_amd/simulate.py restate it in numpy.
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t hash3(uint64_t seed, uint64_t stream, uint64_t idx) {
  return mix64(mix64(seed + stream * 0xD1B54A32D192ED03ull) ^ idx);
}

// A grid holds fewer than 2^32 threads (a larger one wraps silently): refuse instead.
inline int check_grid(int64_t blocks, int threads, const char *what) {
  if (blocks < 0 || blocks > 0x7FFFFFFFLL || blocks * threads >= (1LL << 32))
    return fail(EPI_ERR_ARG, "%s: batch too large for one launch (%lld workgroups of %d threads)", what, (long long)blocks, threads);
  return EPI_OK;
}

}  // namespace epi

#ifdef __HIPCC__
#include "scan.hpp"   // wave, workgroup and device scans, wave_sum_u32: device code, for every .hip unit
#endif
