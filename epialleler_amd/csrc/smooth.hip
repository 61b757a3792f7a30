// CpG strand merging and local-regression smoothing of a cytosine report (include/epihip.h, epi_cx_merge_strands_dev and
// epi_cx_smooth_dev, has the definitions).  No reference interface is replaced.  Both calls are stateless: they read the
// caller's six CX columns, write columns of the caller, take their scratch for the length of the call and touch no batch.
// All on the call's stream:
//  Merge    k_mg_flag: a thread per row checks the row (order, strand, counts), decides from the row and its predecessor
//           whether it is the '-' row of a pair (dropped: its partner takes the sums), a lone '-' CpG that moves to
//           (q - 1, '+') or one that stays, and counts; util.hip's scan over the kept flags; one read of the scalars; then,
//           and only when every check and the capacity hold, k_mg_emit scatters.
//           Why the output strictly ascends again: a pair's row stands where its '+' row stood.  A moved row (rname, q, '-')
//           -> (rname, q - 1, '+') stays above its predecessor, because it moves only when the predecessor is strictly below
//           (rname, q - 1, '+') -- and whatever the predecessor itself becomes is not above what it was -- and it stays below
//           its successor, which was above (rname, q, '-') and hence at (rname, q', .) with q' > q or on a later rname; if
//           the successor moves or is a pair's '+' row it ends at q' - 1 >= q > q - 1 or stays.
//  Smooth   (the series order and its cuts: cx_series.hpp, shared with segment.hip)
//           series_sort: k_series_key checks the rows and writes (class byte, row) pairs; one stable radix pass (radix_sort.hip) brings
//           the rows into series order: the rows of one (strand, context) together, (rname, pos) ascending within.  k_sm_flag
//           gathers pos, meth and coverage into series order and flags the first site of every cluster; the scan over the
//           flags numbers the clusters, k_sm_cstart lists their first sites.  k_smooth_bounds: a thread per site finds D
//           (binary search over the k-wide runs that contain the site), H and the window [jlo, jhi) (two binary searches).
//           One read of the scalars; then k_smooth_fit: a workgroup per SM_TILE consecutive series-ordered sites, a thread
//           per site runs smooth_math.hpp's sums over its window in ascending j and solves -- the host's arithmetic in the
//           host's order inside one thread, so no launch shape is in a result.  pos - H and pos + H do not decrease along a
//           cluster (the k-nearest distance is 1-Lipschitz in pos), and a later cluster's window starts at or behind the end
//           of an earlier one's, so jlo and jhi are monotone over the series order and the workgroup's sites read the one
//           range [jlo(first), jhi(last)): it is staged in LDS once when it holds at most SM_STAGE sites, and read from
//           global memory otherwise (a thread whose window is not inside the staged range reads global memory too: no
//           index depends on the monotonicity).  The same values reach the same operations either way.
#include "cx_series.hpp"
#include "smooth_math.hpp"

namespace epi {

constexpr int SM_WG = 256;
constexpr int SM_TILE = 256;           // sites (threads) of a fit workgroup
constexpr int SM_STAGE = 2048;         // sites of the staged range: 24 KB of LDS
constexpr int32_t CTX_CG = 7;          // the CG context code (api.py's CONTEXT_LEVELS, 1-based)

// ---- merge -------------------------------------------------------------------------------------------------------------

struct MgScalars { uint32_t unsorted, bad, overflow, nrow, nmerged, nmoved, nkept, unused[9]; };
static_assert(sizeof(MgScalars) == 64, "MgScalars layout");

enum { MG_COPY = 0, MG_PAIR_MINUS = 1, MG_MOVE = 2, MG_STAY = 3 };

__device__ __forceinline__ bool mg_minus_cpg(const CxTab &t, uint32_t i) { return t.strand[i] == 2 && t.context[i] == CTX_CG; }

// what row i is: the '-' row of a pair, a lone '-' CpG that moves or stays, or anything else
__device__ __forceinline__ int mg_kind(const CxTab &t, uint32_t i) {
  if (!mg_minus_cpg(t, i)) return MG_COPY;
  const int32_t rname = t.rname[i], q = t.pos[i];
  if (i > 0 && t.rname[i - 1] == rname && (int64_t)t.pos[i - 1] == (int64_t)q - 1 && t.strand[i - 1] == 1 && t.context[i - 1] == CTX_CG)
    return MG_PAIR_MINUS;
  if (q >= 2 && (i == 0 || cx_cmp(t, i - 1, rname, q - 1, 1) < 0)) return MG_MOVE;
  return MG_STAY;
}

__global__ __launch_bounds__(SM_WG) void k_mg_flag(CxTab t, uint32_t *__restrict__ keep, MgScalars *__restrict__ sc) {
  const uint32_t i = blockIdx.x * (uint32_t)SM_WG + threadIdx.x;
  uint32_t merged = 0, moved = 0, kept = 0;
  if (i < t.n) {
    const int32_t strand = t.strand[i], m = t.meth[i], u = t.unmeth[i];
    if (i > 0 && !cx_above(t, i)) atomicOr(&sc->unsorted, 1u);
    if ((strand != 1 && strand != 2) || m < 0 || u < 0) atomicOr(&sc->bad, 1u);
    const int kind = mg_kind(t, i);
    if (kind == MG_PAIR_MINUS) {
      merged = 1;
      if ((int64_t)m + (int64_t)t.meth[i - 1] > 0x7FFFFFFFLL || (int64_t)u + (int64_t)t.unmeth[i - 1] > 0x7FFFFFFFLL) atomicOr(&sc->overflow, 1u);
    }
    moved = kind == MG_MOVE ? 1u : 0u;
    kept = kind == MG_STAY ? 1u : 0u;
    keep[i] = kind == MG_PAIR_MINUS ? 0u : 1u;
  }
  const uint32_t wm = wave_sum_u32(merged), wv = wave_sum_u32(moved), wk = wave_sum_u32(kept);   // (every lane of the wave is here)
  if ((threadIdx.x & 63) == 0) {
    if (wm) atomicAdd(&sc->nmerged, wm);
    if (wv) atomicAdd(&sc->nmoved, wv);
    if (wk) atomicAdd(&sc->nkept, wk);
  }
}

struct MgOut { int32_t *rname, *strand, *pos, *context, *meth, *unmeth; uint32_t nrow; };

__global__ __launch_bounds__(SM_WG) void k_mg_emit(CxTab t, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ off, MgOut o) {
  const uint32_t i = blockIdx.x * (uint32_t)SM_WG + threadIdx.x;
  if (i >= t.n || !keep[i]) return;
  const uint32_t r = off[i];
  if (r >= o.nrow) return;
  int32_t strand = t.strand[i], pos = t.pos[i], m = t.meth[i], u = t.unmeth[i];
  if (i + 1 < t.n && mg_kind(t, i + 1) == MG_PAIR_MINUS) {    // (this row is '+' CG: its own kind is MG_COPY)
    m += t.meth[i + 1]; u += t.unmeth[i + 1];
  } else if (mg_kind(t, i) == MG_MOVE) {
    strand = 1; pos -= 1;
  }
  o.rname[r] = t.rname[i]; o.strand[r] = strand; o.pos[r] = pos; o.context[r] = t.context[i]; o.meth[r] = m; o.unmeth[r] = u;
}

struct MgCounts { int64_t *nrow, *nmerged, *nmoved, *nkept; };

static int cx_merge(epi_engine *e, const CxTab &t, int32_t *const d_out[6], int64_t cap, hipStream_t s, MgCounts c) {
  const char *who = "epi_cx_merge_strands_dev";
  const int64_t n = t.n, nblk = (n + SM_WG - 1) / SM_WG;
  EPI_TRY(check_grid(nblk, SM_WG, "strand merging kernels"));
  CxKeepScratch w;                                            // keep flags and their scan
  EPI_TRY(w.take(n, 2));
  MgScalars *sc = reinterpret_cast<MgScalars *>(w.scal);
  uint32_t *keep = w.flag, *off = keep + n;
  EPI_HIP(hipMemsetAsync(sc, 0, 64, s));
  prof_begin("cxmerge_flag", s);
  hipLaunchKernelGGL(k_mg_flag, dim3((unsigned)nblk), dim3(SM_WG), 0, s, t, keep, sc);
  const int rc_scan = scan_exclusive_u32(keep, off, n, &sc->nrow, w.scan_tmp, s);
  prof_end("cxmerge_flag", s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(rc_scan);
  MgScalars h;                                                // the one synchronisation before anything is written
  EPI_TRY(read_scalars(e, s, sc, sizeof(h), &h));
  if (h.unsorted) return fail(EPI_ERR_ARG, "%s: the rows of the table are not strictly ascending in (rname, pos, strand)", who);
  if (h.bad) return fail(EPI_ERR_ARG, "%s: a row has a strand other than 1 and 2 or a negative count", who);
  if (h.overflow) return fail(EPI_ERR_ARG, "%s: the summed meth or unmeth of a CpG exceeds 2^31 - 1, which an int32 column cannot hold", who);
  *c.nrow = h.nrow; *c.nmerged = h.nmerged; *c.nmoved = h.nmoved; *c.nkept = h.nkept;
  EPI_TRY(cx_rows_fit(who, "rows", h.nrow, cap));
  EPI_TRY(cx_cols_arg(who, d_out, 6, nullptr, 0));
  MgOut o;
  o.rname = d_out[0]; o.strand = d_out[1]; o.pos = d_out[2]; o.context = d_out[3]; o.meth = d_out[4]; o.unmeth = d_out[5];
  o.nrow = h.nrow;
  prof_begin("cxmerge_emit", s);
  hipLaunchKernelGGL(k_mg_emit, dim3((unsigned)nblk), dim3(SM_WG), 0, s, t, keep, off, o);
  prof_end("cxmerge_emit", s);
  EPI_HIP(hipGetLastError());
  EPI_HIP(hipStreamSynchronize(s));                           // (the scratch goes back when this returns)
  return EPI_OK;
}

// ---- smooth: series order, clusters, windows -----------------------------------------------------------------------------

struct SmScalars { uint32_t unsorted, bad, ncluster, max_window, unused[12]; };
static_assert(sizeof(SmScalars) == 64, "SmScalars layout");

struct SmSeries {                      // the table in series order
  int32_t *pos, *meth;
  uint32_t *cov;                       // meth + unmeth
  uint32_t n;
};

__global__ __launch_bounds__(SM_WG) void k_sm_flag(CxTab t, const uint64_t *__restrict__ key, const uint32_t *__restrict__ ord, int32_t max_gap,
                                                   SmSeries o, uint32_t *__restrict__ flag) {
  const uint32_t s = blockIdx.x * (uint32_t)SM_WG + threadIdx.x;
  if (s >= t.n) return;
  const uint32_t row = ord[s];
  const int32_t pos = t.pos[row], m = t.meth[row];
  o.pos[s] = pos; o.meth[s] = m; o.cov[s] = (uint32_t)m + (uint32_t)t.unmeth[row];
  flag[s] = series_head(t, key, ord, s, row, pos, max_gap);
}

// cstart[c]: the first site of cluster c; cstart[ncluster] = n
__global__ __launch_bounds__(SM_WG) void k_sm_cstart(const uint32_t *__restrict__ flag, const uint32_t *__restrict__ off, uint32_t n,
                                                     uint32_t *__restrict__ cstart) {
  const uint32_t s = blockIdx.x * (uint32_t)SM_WG + threadIdx.x;
  if (s >= n) return;
  if (flag[s]) cstart[off[s]] = s;
  if (s == n - 1) cstart[off[s] + flag[s]] = n;
}

struct SmWin { int32_t *H; uint32_t *jlo, *jhi; };

__global__ __launch_bounds__(SM_WG) void k_smooth_bounds(const int32_t *__restrict__ pos, const uint32_t *__restrict__ flag,
                                                         const uint32_t *__restrict__ off, const uint32_t *__restrict__ cstart, uint32_t n,
                                                         int32_t min_sites, int32_t bandwidth, SmWin w, SmScalars *__restrict__ sc) {
  __shared__ uint32_t l_max;
  if (threadIdx.x == 0) l_max = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * (uint32_t)SM_WG + threadIdx.x;
  if (i < n) {
    const uint32_t cid = off[i] + flag[i] - 1u;                // (site 0 is flagged)
    const int64_t lo = cstart[cid], hi = cstart[cid + 1];      // the cluster: [lo, hi), lo <= i < hi
    const int64_t k = hi - lo < (int64_t)min_sites ? hi - lo : (int64_t)min_sites;
    const int64_t pi = pos[i];
    // the k-wide runs [a, a + k) that contain i: a from a_lo to a_hi.  left(a) = pi - pos[a] falls and right(a) =
    // pos[a + k - 1] - pi rises with a; D = min over a of max(left, right) lies where they cross.
    const int64_t a_lo = (int64_t)i - k + 1 > lo ? (int64_t)i - k + 1 : lo, a_hi = (int64_t)i < hi - k ? (int64_t)i : hi - k;
    int64_t x = a_lo, y = a_hi + 1;                            // the smallest a with left(a) <= right(a), or a_hi + 1
    while (x < y) {
      const int64_t mid = x + (y - x) / 2;
      if (pi - (int64_t)pos[mid] <= (int64_t)pos[mid + k - 1] - pi) y = mid; else x = mid + 1;
    }
    int64_t D = 0x7FFFFFFFFFFFFFFFLL;
    if (x <= a_hi) D = (int64_t)pos[x + k - 1] - pi;
    if (x > a_lo) { const int64_t l = pi - (int64_t)pos[x - 1]; D = l < D ? l : D; }
    const int64_t H = D > (int64_t)bandwidth ? D : (int64_t)bandwidth;
    x = lo; y = i;                                             // jlo: the first j with pi - pos[j] < H
    while (x < y) {
      const int64_t mid = x + (y - x) / 2;
      if (pi - (int64_t)pos[mid] < H) y = mid; else x = mid + 1;
    }
    const int64_t jlo = x;
    x = (int64_t)i + 1; y = hi;                                // jhi: the first j with pos[j] - pi >= H
    while (x < y) {
      const int64_t mid = x + (y - x) / 2;
      if ((int64_t)pos[mid] - pi >= H) y = mid; else x = mid + 1;
    }
    w.H[i] = (int32_t)H; w.jlo[i] = (uint32_t)jlo; w.jhi[i] = (uint32_t)x;
    atomicMax(&l_max, (uint32_t)(x - jlo));
  }
  __syncthreads();
  if (threadIdx.x == 0 && l_max) atomicMax(&sc->max_window, l_max);
}

// ---- smooth: the fit -------------------------------------------------------------------------------------------------------

struct SmOut { int32_t *icol[9]; double *dcol[3]; };

template <bool kStage>
__global__ __launch_bounds__(SM_TILE) void k_smooth_fit(CxTab t, const uint32_t *__restrict__ ord, SmSeries ser, SmWin w, int32_t degree, SmOut o) {
  __shared__ int32_t l_pos[kStage ? SM_STAGE : 1], l_meth[kStage ? SM_STAGE : 1];
  __shared__ uint32_t l_cov[kStage ? SM_STAGE : 1];
  const uint32_t s0 = blockIdx.x * (uint32_t)SM_TILE, s = s0 + threadIdx.x;
  uint32_t base = 0, end = 0;
  bool staged = false;
  if (kStage) {                                                // (uniform over the workgroup)
    const uint32_t last = (s0 + SM_TILE < ser.n ? s0 + SM_TILE : ser.n) - 1u;
    base = w.jlo[s0]; end = w.jhi[last];
    staged = end > base && end - base <= (uint32_t)SM_STAGE && end <= ser.n;
    if (staged) {
      for (uint32_t k = threadIdx.x; k < end - base; k += SM_TILE) {
        l_pos[k] = ser.pos[base + k]; l_meth[k] = ser.meth[base + k]; l_cov[k] = ser.cov[base + k];
      }
    }
    __syncthreads();
  }
  if (s >= ser.n) return;
  const uint32_t jlo = w.jlo[s], jhi = w.jhi[s];
  const int32_t Hi = w.H[s];
  const double H = (double)Hi;
  const int64_t pi = ser.pos[s];
  smooth::Sums sum;
  smooth::sums_zero(sum);
  if (kStage && staged && jlo >= base && jhi <= end) {
    for (uint32_t j = jlo - base; j < jhi - base; j++) smooth::sums_add(sum, (int64_t)l_pos[j] - pi, H, l_meth[j], l_cov[j]);
  } else {
    for (uint32_t j = jlo; j < jhi; j++) smooth::sums_add(sum, (int64_t)ser.pos[j] - pi, H, ser.meth[j], ser.cov[j]);
  }
  int used = 0;
  const double sm = smooth::solve(sum, degree, &used);
  const uint32_t row = ord[s];
  const int32_t m = t.meth[row], u = t.unmeth[row];
  o.icol[0][row] = t.rname[row]; o.icol[1][row] = t.strand[row]; o.icol[2][row] = t.pos[row]; o.icol[3][row] = t.context[row];
  o.icol[4][row] = m; o.icol[5][row] = u;
  o.icol[6][row] = (int32_t)(jhi - jlo); o.icol[7][row] = Hi; o.icol[8][row] = used;
  o.dcol[0][row] = (double)m / (double)((int64_t)m + (int64_t)u);
  o.dcol[1][row] = sm;
  o.dcol[2][row] = sum.S0;
}

// ---- host --------------------------------------------------------------------------------------------------------------

// The call's scratch, which epi_cx_smooth_scratch_bytes states: the sort's workspace; pos, meth, coverage in series order, H, jlo, jhi
// and the cluster starts (7 n + 1 words, rounded to 8 bytes); the scalars; the scan's block sums (the sort's table has fewer)
struct SmLayout : ScratchArena {
  size_t sort, words, scal, scan;
  explicit SmLayout(int64_t n) {
    sort = reserve(SortPairs::bytes((size_t)n)); words = reserve(((size_t)n * 7 + 1) * 4, 8); scal = reserve(64); scan = reserve(scan_tmp_bytes(n));
  }
};

struct SmCall { int32_t bandwidth, min_sites, max_gap, degree; int32_t *const *icols; double *const *dcols; };

static int cx_smooth(epi_engine *e, const CxTab &t, const SmCall &c, hipStream_t s, int64_t *ncluster_out, int64_t *max_window_out) {
  const char *who = "epi_cx_smooth_dev";
  const int64_t n = t.n, nblk = (n + SM_WG - 1) / SM_WG;
  EPI_TRY(check_grid(nblk, SM_WG, "smoothing kernels"));
  SmLayout lay(n);                                            // (goes when the call returns)
  EPI_TRY(lay.alloc());
  uint64_t *sort_mem; int32_t *words; SmScalars *sc; uint32_t *scan;
  EPI_TRY(lay.at(lay.sort, &sort_mem)); EPI_TRY(lay.at(lay.words, &words)); EPI_TRY(lay.at(lay.scal, &sc)); EPI_TRY(lay.at(lay.scan, &scan));
  SortPairs sort(sort_mem, (size_t)n);
  DevBuf scan_tmp = DevBuf::view(scan, scan_tmp_bytes(n));
  SmSeries ser;
  ser.pos = words; ser.meth = words + n; ser.cov = reinterpret_cast<uint32_t *>(words + 2 * n); ser.n = (uint32_t)n;
  SmWin w;
  w.H = words + 3 * n; w.jlo = reinterpret_cast<uint32_t *>(words + 4 * n); w.jhi = reinterpret_cast<uint32_t *>(words + 5 * n);
  uint32_t *cstart = reinterpret_cast<uint32_t *>(words + 6 * n);          // n + 1 entries
  EPI_HIP(hipMemsetAsync(sc, 0, 64, s));
  EPI_TRY(series_sort(t, sort, &sc->unsorted, &sc->bad, scan_tmp, "smooth_sort", s));

  const uint32_t *ord = sort.vals();
  uint32_t *flag = sort.spare<uint32_t>(), *off = flag + n;
  prof_begin("smooth_bounds", s);
  hipLaunchKernelGGL(k_sm_flag, dim3((unsigned)nblk), dim3(SM_WG), 0, s, t, sort.keys(), ord, c.max_gap, ser, flag);
  const int rc_scan = scan_exclusive_u32(flag, off, n, &sc->ncluster, scan_tmp, s);
  hipLaunchKernelGGL(k_sm_cstart, dim3((unsigned)nblk), dim3(SM_WG), 0, s, flag, off, (uint32_t)n, cstart);
  hipLaunchKernelGGL(k_smooth_bounds, dim3((unsigned)nblk), dim3(SM_WG), 0, s, ser.pos, flag, off, cstart, (uint32_t)n, c.min_sites, c.bandwidth, w, sc);
  prof_end("smooth_bounds", s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(rc_scan);

  SmScalars h;                                                // the one synchronisation before anything is written
  EPI_TRY(read_scalars(e, s, sc, sizeof(h), &h));
  EPI_TRY(series_verdict(who, h.unsorted, h.bad));
  *ncluster_out = h.ncluster;
  *max_window_out = h.max_window;
  if (h.max_window > (uint32_t)EPI_SMOOTH_MAX_WINDOW)
    return fail(EPI_ERR_ARG, "%s: a window holds %u sites, at most %d (bandwidth = %d, min_sites = %d)", who, h.max_window, EPI_SMOOTH_MAX_WINDOW,
                c.bandwidth, c.min_sites);
  SmOut o;
  for (int i = 0; i < 9; i++) o.icol[i] = c.icols[i];
  for (int i = 0; i < 3; i++) o.dcol[i] = c.dcols[i];
  const int64_t nfit = (n + SM_TILE - 1) / SM_TILE;
  prof_begin("smooth_fit", s);
#ifdef EPI_SMOOTH_GLOBAL_ONLY
  hipLaunchKernelGGL(k_smooth_fit<false>, dim3((unsigned)nfit), dim3(SM_TILE), 0, s, t, ord, ser, w, c.degree, o);
#else
  hipLaunchKernelGGL(k_smooth_fit<true>, dim3((unsigned)nfit), dim3(SM_TILE), 0, s, t, ord, ser, w, c.degree, o);
#endif
  prof_end("smooth_fit", s);
  EPI_HIP(hipGetLastError());
  EPI_HIP(hipStreamSynchronize(s));                           // (the scratch goes back when this returns)
  return EPI_OK;
}

}  // namespace epi

using namespace epi;

extern "C" {

int epi_cx_merge_strands_dev(epi_engine *e, const int32_t *const d_in[6], int64_t n, int32_t *const d_out[6], int64_t cap, void *stream,
                             int64_t *nrow_out, int64_t *nmerged_out, int64_t *nmoved_out, int64_t *nkept_out) {
  const char *who = "epi_cx_merge_strands_dev";
  if (!e || !nrow_out || !nmerged_out || !nmoved_out || !nkept_out) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  *nrow_out = 0; *nmerged_out = 0; *nmoved_out = 0; *nkept_out = 0;
  CxTab t;
  EPI_TRY(cx_tab_arg(who, d_in, n, kCxMaxRows, &t, cap));
  if (cap > 0 && !d_out) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  if (n == 0) return EPI_OK;
  EPI_HIP(hipSetDevice(e->device));
  MgCounts c = {nrow_out, nmerged_out, nmoved_out, nkept_out};
  return cx_merge(e, t, d_out, cap, reinterpret_cast<hipStream_t>(stream), c);
}

int epi_smooth_tile_sites(void) { return SM_TILE; }
int epi_smooth_stage_sites(void) { return SM_STAGE; }

int epi_cx_smooth_scratch_bytes(int64_t n, int64_t *bytes_out) {
  if (!bytes_out) return fail(EPI_ERR_ARG, "epi_cx_smooth_scratch_bytes: NULL argument");
  *bytes_out = 0;
  EPI_TRY(cx_rows_arg("epi_cx_smooth_scratch_bytes", n, kCxMaxRows));
  if (n > 0) *bytes_out = (int64_t)SmLayout(n).used;
  return EPI_OK;
}

int epi_cx_smooth_dev(epi_engine *e, const int32_t *const d_in[6], int64_t n, int32_t bandwidth, int32_t min_sites, int32_t max_gap,
                      int32_t degree, int32_t *const d_icols[9], double *const d_dcols[3], void *stream, int64_t *ncluster_out,
                      int64_t *max_window_out) {
  const char *who = "epi_cx_smooth_dev";
  if (!ncluster_out || !max_window_out) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  *ncluster_out = 0; *max_window_out = 0;
  if (degree < 0 || degree > EPI_SMOOTH_MAX_DEGREE) return fail(EPI_ERR_ARG, "%s: degree = %d, from 0 to %d", who, degree, EPI_SMOOTH_MAX_DEGREE);
  if (bandwidth < 1 || bandwidth > EPI_SMOOTH_MAX_BANDWIDTH)
    return fail(EPI_ERR_ARG, "%s: bandwidth = %d, from 1 to %d", who, bandwidth, EPI_SMOOTH_MAX_BANDWIDTH);
  if (max_gap < 0) return fail(EPI_ERR_ARG, "%s: negative max_gap", who);
  if (min_sites < 1 || min_sites > EPI_SMOOTH_MAX_WINDOW)
    return fail(EPI_ERR_ARG, "%s: min_sites = %d, from 1 to %d", who, min_sites, EPI_SMOOTH_MAX_WINDOW);
  CxTab t;
  EPI_TRY(cx_tab_arg(who, d_in, n, kCxMaxRows, &t));
  if (!e) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  if (n == 0) return EPI_OK;
  EPI_TRY(cx_cols_arg(who, d_icols, 9, d_dcols, 3));
  EPI_HIP(hipSetDevice(e->device));
  SmCall c = {bandwidth, min_sites, max_gap, degree, d_icols, d_dcols};
  return cx_smooth(e, t, c, reinterpret_cast<hipStream_t>(stream), ncluster_out, max_window_out);
}

}  // extern "C"
