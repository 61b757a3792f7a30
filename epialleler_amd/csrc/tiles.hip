// Tile index over the sorted rows.
//
// Positions are cut into tiles of T positions (kTile for CX, kMhlTile for lMHL) on an ABSOLUTE grid (so every GPU of a
// sharded run agrees on tile boundaries).  A tile (rname, t) exists iff some
// row of that rname could reach it: tile(start) <= t <= tile(start + Lmax - 1).
// Because rows are sorted by (rname,start), row x only has to create the tiles
// its predecessor did not already reach -- a purely local count -- and one
// exclusive scan over the rows turns the counts into tile slots; a tile's last
// candidate row is found the same way (row_tiles below).  This replaces
// the reference's "flush the map when start > max_pos" windowing
// (src/rcpp_cx_report.cpp:113) and the key sort of a sort+segmented-reduce
// scheme: the input order already is the sort.
#include "mhl_common.hpp"   // (common.hpp; the lMHL kernels' slab constants for slab_shape)
#include <stdlib.h>
#include <string.h>

namespace epi {

// T is a power of two: tile index by shift (sh = log2 T)
__device__ __forceinline__ int64_t tile_of(int64_t pos, int32_t sh) { return (pos + kPosBias) >> sh; }

__global__ __launch_bounds__(256) void k_row_stats(const int32_t *__restrict__ start, const int32_t *__restrict__ rname,
                                                    const int32_t *__restrict__ strand, const int64_t *__restrict__ off,
                                                    int64_t n, RowStats *__restrict__ st, int32_t *__restrict__ len_out) {
  __shared__ uint32_t s_hist[kLenBinCount];
  if (threadIdx.x < kLenBinCount) s_hist[threadIdx.x] = 0;
  __syncthreads();
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int len = 0, unsorted = 0, bad_strand = 0, bad_len = 0, deep = 0;
  if (x < n) {
    const int64_t l = off[x + 1] - off[x];                  // (the constructors take rows back to back)
    const int32_t s0 = start[x];
    if (l < 0 || (int64_t)s0 + l > 0x7FFFFFFFLL) bad_len = 1; else len = (int)l;
    len_out[x] = len;                                       // the row lengths every later kernel reads (0 for a bad row: the first report raises the error)
    const int32_t sd = strand[x];
    if (sd != 1 && sd != 2 && l != 0) bad_strand = 1;       // (an empty row may carry strand 0: the placeholder template the
                                                            // reference pushes for a paired-end file without a usable pair,
                                                            // src/rcpp_read_bam.cpp:155; it has no bases to count)
    if (x > 0) {
      const int32_t r0 = rname[x - 1], r1 = rname[x];
      if (r1 < r0 || (r1 == r0 && s0 < start[x - 1])) unsorted = 1;
    }
    // Rows covering a position p are consecutive-ish in the sorted order: if x is the first of them, all of them start
    // before start[x] + len[x].  So when row x + 255 starts at or behind the end of row x (for every x), no position is
    // covered by more than 255 rows, and u8 counters per position cannot overflow (cx_report.hip, LEAN).
    if (len > 0 && x + 255 < n && rname[x + 255] == rname[x] && (int64_t)start[x + 255] < (int64_t)s0 + len) deep = 1;
    if (len > 0) {
      const int ch = (len + 30) >> 4;
      int k = 0;
      while (k < kLenBinCount - 1 && ch > kLenBins[k]) k++;
      atomicAdd(&s_hist[k], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x < kLenBinCount && s_hist[threadIdx.x]) atomicAdd(&st->len_hist[threadIdx.x], s_hist[threadIdx.x]);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    len = max(len, __shfl_xor(len, d, 64));
    unsorted |= __shfl_xor(unsorted, d, 64);
    bad_strand |= __shfl_xor(bad_strand, d, 64);
    bad_len |= __shfl_xor(bad_len, d, 64);
    deep |= __shfl_xor(deep, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    // uniform-length input: after the first few waves the cached maximum already covers `len`
    if (len > __hip_atomic_load(&st->max_len, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&st->max_len, len);   // read from L2
    if (unsorted) atomicOr(&st->unsorted, 1);
    if (bad_strand) atomicOr(&st->bad_strand, 1);
    if (bad_len) atomicOr(&st->bad_len, 1);
    if (deep) atomicOr(&st->deep, 1);
  }
}

// What row x contributes to the tile table, from its own and its predecessor's (rname, start) alone:
//  * the tiles it creates, (lo .. b]: those it can reach that its predecessor could not (see header comment);
//  * the tiles it closes, [hi_a .. hi_b]: row_hi of a tile (r,t) is the first row whose (rname, tile of start) lies
//    beyond (r,t).  If x is such a row for anything, it is so exactly for the tiles from its predecessor's start
//    tile up to the predecessor's reach (capped below x's own start tile within one rname) -- tiles the predecessor
//    itself reaches, so they exist, and they are the LAST tiles created before x: their slots count back from the
//    exclusive scan at x.  No search over rows is needed for either end of a tile's row range.
struct RowTiles {
  int64_t lo, b;          // creates tiles lo..b (b < lo: none)
  int64_t hi_a, hi_b, bp; // closes tiles hi_a..hi_b (hi_b < hi_a: none); bp = predecessor's last reachable tile
};

// (s, r) = start / rname of the row, (sp, rp) = of its predecessor (has_prev: the row is not the first of the table)
__device__ __forceinline__ RowTiles row_tiles(int64_t s, int32_t r, int64_t sp, int32_t rp, bool has_prev, int32_t lmax, int32_t sh) {
  RowTiles rt;
  const int64_t sx = tile_of(s, sh);
  rt.b = tile_of(s + lmax - 1, sh);
  rt.lo = sx;
  rt.hi_a = 0; rt.hi_b = -1; rt.bp = 0;
  if (has_prev) {
    const int64_t tp = tile_of(sp, sh);
    rt.bp = tile_of(sp + lmax - 1, sh);
    if (rp == r) {
      if (rt.bp + 1 > rt.lo) rt.lo = rt.bp + 1;
      if (sx != tp) { rt.hi_a = tp; rt.hi_b = rt.bp < sx - 1 ? rt.bp : sx - 1; }
    } else {
      rt.hi_a = tp; rt.hi_b = rt.bp;
    }
  }
  return rt;
}

// The tile table in two passes over (start, rname) with nothing stored per row in between: pass A (FILL = false)
// reduces the per-row tile counts of a block of TB_ROWS rows to one number; after a single-block scan of those
// (scan_block_sums_inplace) pass B (FILL = true) recomputes the counts, scans them inside the block and writes the tiles.
// A thread owns TB_ITEMS CONSECUTIVE rows: four 16-byte loads bring their columns, a row's predecessor is the
// thread's previous row, and the scan in row order is a serial prefix inside the thread plus one wavefront scan of
// the thread totals (the first version strided the rows over the threads: 32 scalar loads and eight wavefront scans
// per thread, 51-67 us for 10 M rows against 30).
constexpr int TB_THREADS = 256, TB_ITEMS = 8, TB_ROWS = TB_THREADS * TB_ITEMS;

struct __attribute__((packed, aligned(4))) TileI4 { int32_t v[4]; };   // 16 bytes at int32 alignment (adopted columns may be views)

// VERIFY (with FILL): `bsum` is the scanned block-sum array remembered from an earlier call on this batch and tile
// size (the count pass, the scan and the host round trip are skipped); every block checks its own total against it and
// the table's capacity `cap` is the remembered tile count.  sc->ntiles (zeroed before the launch) ends up as that count,
// or as 0xFFFFFFFF when any block disagrees -- the rows were changed under the batch -- which the caller reports.
template <bool FILL, bool VERIFY = false>
__global__ __launch_bounds__(TB_THREADS) void k_tile_pass(const int32_t *__restrict__ start, const int32_t *__restrict__ rname,
                                                           int64_t n, int32_t lmax, int32_t sh, uint32_t *__restrict__ bsum,
                                                           Tile *__restrict__ tiles, const int64_t *__restrict__ shared_keys,
                                                           int32_t nshared, int32_t *__restrict__ slot_tile,
                                                           Scalars *__restrict__ sc, int64_t cap) {
  // (cap = entries of `tiles`: the count may be one remembered from an earlier call -- a batch that was changed since
  //  must not write behind the table before the host notices)
  __shared__ uint32_t s_tot[TB_THREADS / 64];
  if (FILL && blockIdx.x == 0 && threadIdx.x == 0) {       // the report kernels' counters start at zero (saves three memsets)
    sc->cursor = 0; sc->rows = 0; sc->heavy_count = 0; sc->heavy_max = 0;
    sc->deep_count = 0;
    sc->fold_cursor = 0;
  }
  const int64_t x0 = (int64_t)blockIdx.x * TB_ROWS + (int64_t)threadIdx.x * TB_ITEMS;
  int32_t st[TB_ITEMS + 1], rn[TB_ITEMS + 1];              // [0] = the predecessor of the thread's first row
#pragma unroll
  for (int i = 0; i <= TB_ITEMS; i++) { st[i] = 0; rn[i] = 0; }
  if (x0 < n) {
    if (x0 > 0) { st[0] = start[x0 - 1]; rn[0] = rname[x0 - 1]; }
    if (x0 + TB_ITEMS <= n) {
#pragma unroll
      for (int q = 0; q < TB_ITEMS / 4; q++) {
        const TileI4 a = *reinterpret_cast<const TileI4 *>(start + x0 + 4 * q), c = *reinterpret_cast<const TileI4 *>(rname + x0 + 4 * q);
#pragma unroll
        for (int k = 0; k < 4; k++) { st[1 + 4 * q + k] = a.v[k]; rn[1 + 4 * q + k] = c.v[k]; }
      }
    } else {
#pragma unroll
      for (int i = 0; i < TB_ITEMS; i++) if (x0 + i < n) { st[1 + i] = start[x0 + i]; rn[1 + i] = rname[x0 + i]; }
    }
  }
  uint32_t c[TB_ITEMS], tot = 0;
#pragma unroll
  for (int i = 0; i < TB_ITEMS; i++) {
    c[i] = 0;
    if (x0 + i < n) {
      const RowTiles rt = row_tiles(st[1 + i], rn[1 + i], st[i], rn[i], x0 + i > 0, lmax, sh);
      if (rt.b >= rt.lo) c[i] = (uint32_t)(rt.b - rt.lo + 1);
    }
    tot += c[i];
  }
  uint32_t btot;
  const uint32_t tbase = wg_scan_excl<SumU32, TB_THREADS>(tot, s_tot, &btot);
  if (!FILL) {
    if (threadIdx.x == 0) bsum[blockIdx.x] = btot;
    return;
  }
  if constexpr (VERIFY) {
    if (threadIdx.x == 0) {
      const uint32_t expect = (blockIdx.x + 1 < gridDim.x ? bsum[blockIdx.x + 1] : (uint32_t)cap) - bsum[blockIdx.x];
      if (btot != expect) atomicMax(&sc->ntiles, 0xFFFFFFFFu);
      else if (blockIdx.x == 0) atomicMax(&sc->ntiles, (uint32_t)cap);
    }
  }
  uint32_t before = bsum[blockIdx.x] + tbase;             // tiles created by rows before the thread's first row
  const int64_t T = 1LL << sh;
#pragma unroll
  for (int i = 0; i < TB_ITEMS; i++) {
    const int64_t x = x0 + i;
    if (x >= n) break;
    const RowTiles rt = row_tiles(st[1 + i], rn[1 + i], st[i], rn[i], x > 0, lmax, sh);
    for (int64_t t = rt.hi_a; t <= rt.hi_b; t++) {          // tiles this row closes
      const int64_t j = (int64_t)before - 1 - (rt.bp - t);
      if (j >= 0 && j < cap) tiles[j].row_hi = (int32_t)x;
    }
    if (c[i]) {
      const int32_t r = rn[1 + i];
      for (uint32_t k = 0; k < c[i]; k++) {                 // tiles this row creates: it IS their row_lo
        const int64_t t = rt.lo + k;                        // (the first row with start >= pos0 - lmax + 1)
        if ((int64_t)before + k >= cap) break;
        Tile *td = tiles + before + k;
        td->pos0 = t * T - kPosBias;
        td->rname = r;
        td->row_lo = (int32_t)x;
        int32_t slot = -1;
        if (nshared > 0) {
          const int64_t key = ((int64_t)r << 32) | (int64_t)(uint32_t)t;
          int32_t a = 0, z = nshared;
          while (a < z) { int32_t m = (a + z) >> 1; if (shared_keys[m] < key) a = m + 1; else z = m; }
          if (a < nshared && shared_keys[a] == key) { slot = a; slot_tile[a] = (int32_t)(before + k); }
        }
        td->slot = slot;
      }
    }
    if (x == n - 1) {                                       // the end of the table closes what the last row reaches
      const int64_t sx = tile_of(st[1 + i], sh);
      for (int64_t t = sx; t <= rt.b; t++) {
        const int64_t j = (int64_t)before + c[i] - 1 - (rt.b - t);
        if (j >= 0 && j < cap) tiles[j].row_hi = (int32_t)n;
      }
    }
    before += c[i];
  }
}

// what the index pass leaves in the scalars when the table itself is reused: the tile count and the report kernels' zeroed counters
__global__ void k_misc_reset(Scalars *__restrict__ sc, const uint32_t *__restrict__ nt) {
  if (threadIdx.x == 0) {
    sc->ntiles = nt[0];
    sc->cursor = 0; sc->rows = 0; sc->heavy_count = 0; sc->deep_count = 0; sc->fold_cursor = 0; sc->heavy_max = 0;
  }
}

static int log2_tile(int32_t T) {
  int sh = 0;
  while ((1 << sh) < T) sh++;
  return sh;
}

// Row statistics are a property of the (immutable) batch: queued once, when the batch is created.
int launch_row_stats(epi_batch *b, hipStream_t s) {
  EPI_TRY(b->stats.ensure(sizeof(RowStats)));
  EPI_TRY(b->own_len.ensure((size_t)b->n * 4 + 4));
  b->len = b->own_len.as<int32_t>();
  EPI_HIP(hipMemsetAsync(b->stats.p, 0, sizeof(RowStats), s));
  if (b->n > 0) {
    const unsigned nb = (unsigned)((b->n + 255) / 256);
    hipLaunchKernelGGL(k_row_stats, dim3(nb), dim3(256), 0, s, b->start, b->rname, b->strand, b->off, b->n, b->stats.as<RowStats>(),
                       b->own_len.as<int32_t>());
    EPI_HIP(hipGetLastError());
  }
  if (!b->stats_done) EPI_HIP(hipEventCreateWithFlags(&b->stats_done, hipEventDisableTiming));
  EPI_HIP(hipEventRecord(b->stats_done, s));
  b->stats_queued = true;
  return EPI_OK;
}

int fetch_row_stats(epi_batch *b, hipStream_t s) {
  if (b->stats_host) return EPI_OK;
  if (!b->stats_queued) EPI_TRY(launch_row_stats(b, s));
  EPI_HIP(hipEventSynchronize(b->stats_done));              // the kernel may sit on another stream than `s`
  EPI_TRY(read_scalars(b, s, b->stats.p, sizeof(RowStats), &b->h_stats));
  b->stats_host = true;
  return EPI_OK;
}

// The slabs of a shared tile, from the kernels' own constants
SlabShape slab_shape(SlabKind kind, int T) {
  switch (kind) {
    case SLAB_CX: return {(size_t)kCxPlanes * T, 0};
    case SLAB_MHL: return {(size_t)MHL_CNT_PLANES * MHL_T, (size_t)MHL_NSUM};
    case SLAB_MHL_FUSED: return {(size_t)MHLF_CNT_PLANES * MHLF_T, (size_t)MHLF_SUM_PLANES * MHLF_T};
    default: return {0, 0};
  }
}

// The shared tile keys of a sharded report and which of them this rank owns (keys strictly increasing), with the slabs their
// tiles add into; nshared = 0: none, nothing attached.  A tile's slot is assigned when the tile table is built.
int attach_shared(epi_batch *b, const int64_t *h_keys, const int32_t *h_owned, int32_t nshared, SlabKind kind, int32_t *d_cnt, int64_t *d_sum) {
  if (!b || nshared < 0 || (nshared > 0 && (!h_keys || !h_owned)))
    return fail(EPI_ERR_ARG, "epi_batch_cx_set_shared: bad arguments");
  for (int32_t i = 1; i < nshared; i++)
    if (h_keys[i - 1] >= h_keys[i]) return fail(EPI_ERR_ARG, "epi_batch_cx_set_shared: keys must be strictly increasing");
  EPI_HIP(hipSetDevice(b->eng->device));
  ShardState &sh = b->shard;
  sh.keys.assign(h_keys, h_keys + nshared);
  sh.owned.assign(h_owned, h_owned + nshared);
  sh.kind = SLAB_NONE; sh.d_cnt = nullptr; sh.d_sum = nullptr;
  if (nshared == 0) return EPI_OK;
  // a sharded run attaches the same keys for every report: skip the copies when the device already holds them
  if (sh.dev_keys != sh.keys || sh.dev_owned != sh.owned) {
    EPI_TRY(sh.d_keys.ensure((size_t)nshared * 8));
    EPI_TRY(sh.d_owned.ensure((size_t)nshared * 4));
    EPI_HIP(hipMemcpy(sh.d_keys.p, h_keys, (size_t)nshared * 8, hipMemcpyHostToDevice));
    EPI_HIP(hipMemcpy(sh.d_owned.p, h_owned, (size_t)nshared * 4, hipMemcpyHostToDevice));
    sh.dev_keys = sh.keys;
    sh.dev_owned = sh.owned;
  }
  sh.kind = kind; sh.d_cnt = d_cnt; sh.d_sum = d_sum;
  return EPI_OK;
}

int zero_shared_slabs(epi_batch *b, int T, hipStream_t s) {
  const ShardState &sh = b->shard;
  const SlabShape shape = slab_shape(sh.kind, T);
  if (shape.cnt) EPI_HIP(hipMemsetAsync(sh.d_cnt, 0, sh.keys.size() * shape.cnt * 4, s));
  if (shape.sum) EPI_HIP(hipMemsetAsync(sh.d_sum, 0, sh.keys.size() * shape.sum * 8, s));
  return EPI_OK;
}

int finish_shared_rows(epi_batch *b, hipStream_t s, ReportKind done, size_t ovf_base, size_t pool_cap, const char *overflow_msg,
                       int (*deferred)(epi_batch *, const Scalars &), int64_t *nrow_out) {
  Scalars *sc = report_scalars(b);
  EPI_TRY(scan_exclusive_u32(b->pool.tile_nrow.as<uint32_t>(), b->pool.tile_out.as<uint32_t>(), b->last_ntiles, &sc->rows, b->scan_tmp, s));
  Scalars host;                                             // overflow rows handed out, total rows: one sync
  EPI_TRY(read_report_scalars(b, s, &host));
  if (deferred) EPI_TRY(deferred(b, host));
  // cannot overflow: the first half kept 2 T rows per shared tile free
  if (ovf_base + host.cursor > pool_cap) return fail(EPI_ERR_STATE, "%s", overflow_msg);
  b->last_kind = done;
  b->last_nrow = host.rows;
  *nrow_out = host.rows;
  return EPI_OK;
}

// Validated row statistics (errors for bad offsets / strands / unsorted rows) + the tile table for tiles of T
// positions.  One host synchronisation per call (the tile count); the statistics come back with the first one.
int build_tiles(epi_batch *b, hipStream_t s, int32_t T, RowStats *h, int32_t *ntiles_out, bool *hinted) {
  *ntiles_out = 0;
  if (hinted) *hinted = false;
  memset(h, 0, sizeof(*h));
  if ((T & (T - 1)) != 0) return fail(EPI_ERR_ARG, "tile size must be a power of two");
  const int sh = log2_tile(T);
  EPI_TRY(b->misc.ensure(256));
  Scalars *sc = report_scalars(b);
  if (b->n == 0) { EPI_HIP(hipMemsetAsync(sc, 0, offsetof(Scalars, heavy_max) + 4, s)); return EPI_OK; }
  EPI_TRY(fetch_row_stats(b, s));
  *h = b->h_stats;
  if (h->bad_len) return fail(EPI_ERR_ARG, "offsets are not non-decreasing, or start+length exceeds int32");
  if (h->bad_strand) return fail(EPI_ERR_ARG, "strand values must be 1 ('+') or 2 ('-')");
  if (h->unsorted)
    return fail(EPI_ERR_UNSORTED, "rows are not sorted by (rname,start); the reference requires a pre-sorted dataset "
                                  "(src/rcpp_cx_report.cpp:19)");
  const int32_t lmax = h->max_len > 0 ? h->max_len : 1;
  const int64_t nb = (b->n + TB_ROWS - 1) / TB_ROWS;
  EPI_TRY(check_grid(nb, TB_THREADS, "tile index"));
  int slot = -1;
  for (int i = 0; i < 4; i++) if (b->tix.hint[i].T == T) slot = i;
  const int use_hint = options().tile_hint;                // EPIHIP_TILE_HINT=0: every call counts, scans and asks (A/B runs, tests)
  auto remember_table = [&](uint32_t nt) -> int {            // (after the pass that filled b->tix.tiles)
    b->tix.built.T = 0;
    if (!b->cols_owned) return EPI_OK;
    EPI_TRY(b->tix.nt_dev.ensure(4));
    EPI_HIP(hipMemcpyAsync(b->tix.nt_dev.p, &sc->ntiles, 4, hipMemcpyDeviceToDevice, s));
    b->tix.built.T = T; b->tix.built.nt = (int32_t)nt; b->tix.built.lmax = lmax; b->tix.built.shared = b->shard.keys;
    return EPI_OK;
  };
  if (use_hint && hinted && b->cols_owned && b->tix.built.T == T && b->tix.built.lmax == lmax && b->tix.built.shared == b->shard.keys) {
    // the batch owns its columns and the table of the last build was made for this tile size and these shared keys: it is
    // still there (tiles, d_slot_tile); sc->ntiles gets the count the pass had left, which the caller compares as always
    hipLaunchKernelGGL(k_misc_reset, dim3(1), dim3(64), 0, s, sc, b->tix.nt_dev.as<uint32_t>());   // (one launch instead of three copies)
    EPI_HIP(hipGetLastError());
    *hinted = true;
    *ntiles_out = b->tix.built.nt;
    return EPI_OK;
  }
  if (use_hint && hinted && slot >= 0 && b->tix.hint[slot].lmax == lmax) {
    // The tile count and the per-block offsets are functions of the batch's rows and T alone: with those of an earlier
    // call the table is allocated up front and filled by ONE pass that verifies them block by block; the caller
    // compares sc->ntiles with the count when it next synchronises anyway.
    const uint32_t nt = (uint32_t)b->tix.hint[slot].nt;
    EPI_TRY(b->tix.tiles.ensure((size_t)nt * sizeof(Tile)));
    const int32_t nshared = (int32_t)b->shard.keys.size();
    if (nshared > 0) {
      EPI_TRY(b->shard.d_slot_tile.ensure((size_t)nshared * 4));
      EPI_HIP(hipMemsetAsync(b->shard.d_slot_tile.p, 0xFF, (size_t)nshared * 4, s));
    }
    EPI_HIP(hipMemsetAsync(&sc->ntiles, 0, 4, s));
    prof_begin("tile_index", s);
    hipLaunchKernelGGL((k_tile_pass<true, true>), dim3((unsigned)nb), dim3(TB_THREADS), 0, s, b->start, b->rname, b->n, lmax, sh,
                       b->tix.hint[slot].bsum.as<uint32_t>(), b->tix.tiles.as<Tile>(), b->shard.d_keys.as<int64_t>(), nshared,
                       b->shard.d_slot_tile.as<int32_t>(), sc, (int64_t)nt);
    prof_end("tile_index", s);
    EPI_HIP(hipGetLastError());
    EPI_TRY(remember_table(nt));
    *hinted = true;
    *ntiles_out = (int32_t)nt;
    return EPI_OK;
  }
  b->tix.built.T = 0;
  EPI_TRY(b->scan_tmp.ensure((size_t)nb * 4));
  uint32_t *bsum = b->scan_tmp.as<uint32_t>();
  hipLaunchKernelGGL((k_tile_pass<false>), dim3((unsigned)nb), dim3(TB_THREADS), 0, s, b->start, b->rname, b->n, lmax, sh, bsum,
                     (Tile *)nullptr, (const int64_t *)nullptr, 0, (int32_t *)nullptr, sc, (int64_t)0);
  EPI_HIP(hipGetLastError());
  EPI_TRY(scan_block_sums_inplace(bsum, nb, &sc->ntiles, s));
  uint32_t nt = 0;
  EPI_TRY(read_scalars(b, s, &sc->ntiles, 4, &nt));
  if (nt <= 0x7FFFFFF0u) {                                 // remember count and block offsets for the one-pass path above
    for (int i = 0; i < 4 && slot < 0; i++) if (b->tix.hint[i].T == 0) slot = i;
    if (slot >= 0 && b->tix.hint[slot].bsum.ensure((size_t)nb * 4) == EPI_OK &&
        hipMemcpyAsync(b->tix.hint[slot].bsum.p, bsum, (size_t)nb * 4, hipMemcpyDeviceToDevice, s) == hipSuccess) {
      b->tix.hint[slot].T = T; b->tix.hint[slot].nt = (int32_t)nt; b->tix.hint[slot].lmax = lmax;
    }
  }
  if (nt > 0x7FFFFFF0u) return fail(EPI_ERR_ARG, "too many tiles (%u)", nt);
  EPI_TRY(b->tix.tiles.ensure((size_t)nt * sizeof(Tile)));
  const int32_t nshared = (int32_t)b->shard.keys.size();
  if (nshared > 0) {   // slot -> this rank's tile index (-1: this rank has no rows near that tile)
    EPI_TRY(b->shard.d_slot_tile.ensure((size_t)nshared * 4));
    EPI_HIP(hipMemsetAsync(b->shard.d_slot_tile.p, 0xFF, (size_t)nshared * 4, s));
  }
  hipLaunchKernelGGL((k_tile_pass<true>), dim3((unsigned)nb), dim3(TB_THREADS), 0, s, b->start, b->rname, b->n, lmax, sh, bsum,
                     b->tix.tiles.as<Tile>(), b->shard.d_keys.as<int64_t>(), nshared, b->shard.d_slot_tile.as<int32_t>(), sc, (int64_t)nt);
  EPI_HIP(hipGetLastError());
  EPI_TRY(remember_table(nt));
  *ntiles_out = (int32_t)nt;
  return EPI_OK;
}

// Row pool of a report (CX, two-kernel lMHL, one-pass lMHL) = one slot of `slot` rows per tile + an overflow region behind
// the slots, out of which a tile that outgrows its slot takes rows through Scalars::cursor.  The caller remembers a slot
// size per kind of report: it starts at a typical density of reported positions and doubles for the next call when more
// than 1/8 of the rows went through the cursor; an overflow of the region itself is detected after the run and costs one
// rerun with the exact size.  layout_pool clamps the remembered slot to 2 T (a tile has T positions on two strands),
// lets the test hook replace it (hook_slot >= 0), halves it until the slots stay below 0xC0000000 rows (row indices are
// u32), and has `reserve` grow that report's pool to slots + region (1/16 of the slots, at least 65 536 rows) + headroom;
// reserve(b, rows) returns at once when the pool holds `rows` rows already.  Where the slots do not fit in device memory
// the layout falls back to slot = 0: every tile through the cursor, the pool sized by the rows actually produced.
int layout_pool(epi_batch *b, uint32_t slot, int T, int32_t nt, size_t headroom, int hook_slot, int (*reserve)(epi_batch *, size_t rows),
                PoolLayout *out) {
  if (slot > 2u * T) slot = 2u * T;
  if (hook_slot >= 0 && hook_slot <= 2 * T) slot = (uint32_t)hook_slot;
  while (slot && (unsigned long long)nt * slot > 0xC0000000ull) slot >>= 1;
  size_t ovf_base = (size_t)nt * slot;
  for (;;) {
    const size_t ovf = (ovf_base >> 4) > 65536 ? (ovf_base >> 4) : 65536;
    const int rc = reserve(b, ovf_base + ovf + headroom);
    if (rc == EPI_OK) break;
    b->pool.row_cap = 0; b->pool.row_cap2 = 0;                     // (a failed growth has released the old buffers; row_cap2: lMHL's 64-bit columns)
    if (!slot) return rc;
    slot = 0;
    ovf_base = 0;
  }
  out->slot = slot;
  out->ovf_base = ovf_base;
  return EPI_OK;
}

}  // namespace epi
