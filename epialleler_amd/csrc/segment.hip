// Methylation segments of a cytosine report by an HMM with exact Viterbi decoding (include/epihip.h, epi_cx_segment_dev, has
// the model; segment_math.hpp has its arithmetic, shared with the plain loop of segment_host.cpp).  No reference interface is
// replaced.  The call is stateless: it reads the caller's six CX columns, writes columns of the caller, takes its scratch for
// the length of the call and touches no batch.  All on the call's stream, every phase a launch of its own -- no kernel waits
// on another workgroup:
//  Order     cx_series.hpp's series_sort (the row checks and class byte, one stable radix pass), k_sg_gather: the sites in series
//            order as one word each (clipped counts m', u' and the chain-head bit, cx_series.hpp's rule).  One read of the
//            scalars: the input's errors end the call here.
//  Forward   a segmented inclusive scan of max-plus matrices.  A site inside a chain is M[j][k] = T[j][k] + e(k); a chain's
//            first site is H[j][k] = I[k] + e(k) for every j and is flagged: a flagged element forgets what stands before it.
//            (a) k_sg_fwd_agg: a thread multiplies the matrices of its SG_T sites, an LDS scan over the workgroup's SG_WG
//            threads gives the workgroup's aggregate.  (b) k_sg_fwd_carry: one workgroup scans the aggregates; site 0 is a
//            head, so every prefix is flagged and its row 0 IS the delta vector behind the workgroup's predecessor: K numbers
//            per workgroup.  (c) k_sg_fwd_walk: (a)'s products and scan again, now for every thread's exclusive prefix; the
//            thread's incoming delta is the carry through that prefix (or the prefix's row 0 when it holds a head), and the
//            thread walks its sites with the K^2 step.  delta is never stored.  Per site i one byte f_i, the map from site
//            i + 1's state to site i's: psi_{i+1}, or at a chain's last site the constant map to the chain's end state (the
//            thread steps one site into its neighbour's range for psi_{i+1}: SG_T + 1 steps for SG_T bytes, all its own).  A
//            chain's score is added where the chain ends: a sum per thread, per workgroup in LDS, one 64-bit atomic per
//            workgroup.  Integer max and + are exactly associative: the deltas, hence every psi and every tie, are the loop's.
//  Backward  a suffix scan of the f bytes under composition, the same three phases (k_sg_bwd_agg, k_sg_bwd_carry,
//            k_sg_bwd_walk).  A constant map forgets what stands behind it, so chains need no flag here; the table's last
//            site ends a chain, so every suffix is constant.  It leaves the states in series order.
//  Refit     k_sg_counts: at most SG_COUNT_WGS workgroups over strided shares of the sites, a thread per site and round, every
//            counter of M, U, N, S summed over the wave (DPP), one LDS add per wave (32-bit: a workgroup's share cannot overflow
//            them), one 64-bit atomic add per counter per workgroup; the host reads the counters once per iteration and
//            re-estimates.
//  Segments  k_sg_runs flags the run starts, util.hip's scan numbers them; one read of the scalars (the score, the number
//            of segments); then, and only when the rows fit: k_sg_emit_sites scatters the states to the row order and writes a
//            row's keys at its run's first site and its end at the last; k_sg_emit_sums adds the raw counts per thread of SG_T
//            sites and run (integer atomics: exact in any order); k_sg_emit_rows turns the sums into doubles.  No thread walks
//            a whole run (a thread per run start doing so took two thirds of a decode on long runs: profiles/segment_report.txt).
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN 4.21 has the table; no kernel uses scratch memory.
#include "cx_series.hpp"
#include "segment_math.hpp"

namespace epi {

namespace sg = segment;

constexpr int SG_WG = 256;
constexpr int SG_T = 8;                // sites a thread walks
constexpr int SG_B = SG_WG * SG_T;     // series-ordered sites a workgroup scans
static_assert(SG_T == 8, "a thread's f bytes and states are one 8-byte store");
constexpr int SG_COUNT_WGS = 512;      // workgroups of the counts kernel: a share of 2^26 / 512 sites * 32767 counts = 2^32 - 2^17 fits its LDS counters

struct SgScalars {
  uint32_t unsorted, bad, nchain, nsegment;
  unsigned long long score;            // two's complement sum of the chains' scores
  unsigned long long counts[28];       // M[K], U[K], N[K][K], S[K]
  unsigned long long unused;
};
static_assert(sizeof(SgScalars) == 256 && offsetof(SgScalars, score) == 16, "SgScalars layout");

// ---- series order ------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(SG_WG) void k_sg_gather(CxTab t, const uint64_t *__restrict__ key, const uint32_t *__restrict__ ord, int32_t max_gap,
                                                     int32_t max_coverage, uint32_t *__restrict__ w, SgScalars *__restrict__ sc) {
  const uint32_t s = blockIdx.x * (uint32_t)SG_WG + threadIdx.x;
  uint32_t head = 0;
  if (s < t.n) {
    const uint32_t row = ord[s];
    head = series_head(t, key, ord, s, row, t.pos[row], max_gap);
    int32_t m, u;
    sg::clip_counts(t.meth[row], t.unmeth[row], max_coverage, &m, &u);
    w[s] = sg::site_pack(m, u, head != 0);
  }
  const uint32_t heads = wave_sum_u32(head);                   // (every lane of the wave is here)
  if ((threadIdx.x & 63) == 0 && heads) atomicAdd(&sc->nchain, heads);
}

// a thread's SG_T + 1 site words from site a on; a site outside the table reads as a chain head with no counts
__device__ __forceinline__ void sg_load_sites(const uint32_t *__restrict__ w, uint32_t a, uint32_t n, uint32_t (&x)[SG_T + 1]) {
  if (a + SG_T <= n) {                                         // (a is a multiple of SG_T: 32-byte aligned)
    const uint4 lo = *reinterpret_cast<const uint4 *>(w + a), hi = *reinterpret_cast<const uint4 *>(w + a + 4);
    x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w; x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
  } else {
#pragma unroll
    for (int i = 0; i < SG_T; i++) x[i] = a + (uint32_t)i < n ? w[a + i] : 0x80000000u;
  }
  x[SG_T] = a + SG_T < n ? w[a + SG_T] : 0x80000000u;
}

// ---- forward -------------------------------------------------------------------------------------------------------------

// an element of the forward scan: the product of a run of sites; flag: the run holds a chain head (every row of m is then the
// same: what stood before is forgotten); none: the empty run
template <int K> struct FwdAgg { sg::Mat<K> m; uint32_t flag, none; };

template <int K> __device__ __forceinline__ void fwd_combine(const FwdAgg<K> &a, FwdAgg<K> &b) {   // b <- a, then b
  if (a.none || b.flag) return;
  if (b.none) { b = a; return; }
  sg::maxplus<K>(a.m, b.m, b.m);
  b.flag = a.flag;
}

// the product of the thread's sites x[0 .. SG_T), in order
template <int K> __device__ __forceinline__ void fwd_thread_agg(const sg::Tables &t, const uint32_t (&x)[SG_T + 1], uint32_t a, uint32_t n, FwdAgg<K> &g) {
  g.flag = 0; g.none = 1;
#pragma unroll
  for (int k = 0; k < K * K; k++) g.m.a[k] = 0;
#pragma unroll
  for (int i = 0; i < SG_T; i++) {
    if (a + (uint32_t)i < n) {
      sg::Vec<K> e;
      sg::Mat<K> m;
      const bool head = sg::site_head(x[i]);
      sg::emission<K>(t, sg::site_m(x[i]), sg::site_u(x[i]), e);
      sg::site_matrix<K>(t, e, head, m);
      if (g.none || head) { g.m = m; g.flag = head ? 1u : 0u; g.none = 0; }
      else sg::maxplus<K>(g.m, m, g.m);
    }
  }
}

// Inclusive scan over the workgroup's threads in LDS (Hillis-Steele: 8 rounds, each thread reads its partner, waits, combines
// and writes); on return buf[tid] holds thread tid's inclusive prefix.
template <int K> __device__ __forceinline__ void fwd_wg_scan(FwdAgg<K> &mine, FwdAgg<K> *buf) {
  const uint32_t tid = threadIdx.x;
  buf[tid] = mine;
  __syncthreads();
#pragma unroll 1
  for (uint32_t d = 1; d < (uint32_t)SG_WG; d <<= 1) {
    FwdAgg<K> other;
    other.none = 1; other.flag = 0;
    if (tid >= d) other = buf[tid - d];
    __syncthreads();
    if (tid >= d) { fwd_combine<K>(other, mine); buf[tid] = mine; }
    __syncthreads();
  }
}

template <int K>
__global__ __launch_bounds__(SG_WG) void k_sg_fwd_agg(const uint32_t *__restrict__ w, uint32_t n, sg::Tables t, FwdAgg<K> *__restrict__ blkagg) {
  __shared__ FwdAgg<K> buf[SG_WG];
  const uint32_t a = blockIdx.x * (uint32_t)SG_B + threadIdx.x * (uint32_t)SG_T;
  uint32_t x[SG_T + 1];
  sg_load_sites(w, a, n, x);
  FwdAgg<K> g;
  fwd_thread_agg<K>(t, x, a, n, g);
  fwd_wg_scan<K>(g, buf);
  if (threadIdx.x == SG_WG - 1) blkagg[blockIdx.x] = g;
}

// one workgroup: carry[b] = the delta vector behind the last site in front of workgroup b (b >= 1; carry[0] is not used)
template <int K>
__global__ __launch_bounds__(SG_WG) void k_sg_fwd_carry(const FwdAgg<K> *__restrict__ blkagg, uint32_t nblk, sg::Vec<K> *__restrict__ carry) {
  __shared__ FwdAgg<K> buf[SG_WG];
  const uint32_t chunk = (nblk + SG_WG - 1) / SG_WG, lo = threadIdx.x * chunk, hi = lo + chunk < nblk ? lo + chunk : nblk;
  FwdAgg<K> g;
  g.none = 1; g.flag = 0;
#pragma unroll
  for (int k = 0; k < K * K; k++) g.m.a[k] = 0;
  for (uint32_t b = lo; b < hi; b++) {
    FwdAgg<K> x = blkagg[b];
    fwd_combine<K>(g, x);
    g = x;
  }
  fwd_wg_scan<K>(g, buf);
  FwdAgg<K> run;
  run.none = 1; run.flag = 0;
#pragma unroll
  for (int k = 0; k < K * K; k++) run.m.a[k] = 0;
  if (threadIdx.x > 0) run = buf[threadIdx.x - 1];
  for (uint32_t b = lo; b < hi; b++) {
    sg::Vec<K> d;
#pragma unroll
    for (int k = 0; k < K; k++) d.v[k] = run.m.a[k];           // row 0 (a flagged product: every row)
    carry[b] = d;
    FwdAgg<K> x = blkagg[b];
    fwd_combine<K>(run, x);
    run = x;
  }
}

template <int K>
__global__ __launch_bounds__(SG_WG) void k_sg_fwd_walk(const uint32_t *__restrict__ w, uint32_t n, sg::Tables t, const sg::Vec<K> *__restrict__ carry,
                                                       uint8_t *__restrict__ fmap, SgScalars *__restrict__ sc) {
  __shared__ FwdAgg<K> buf[SG_WG];
  __shared__ unsigned long long l_score;
  if (threadIdx.x == 0) l_score = 0;
  const uint32_t a = blockIdx.x * (uint32_t)SG_B + threadIdx.x * (uint32_t)SG_T;
  uint32_t x[SG_T + 1];
  sg_load_sites(w, a, n, x);
  {
    FwdAgg<K> g;
    fwd_thread_agg<K>(t, x, a, n, g);
    fwd_wg_scan<K>(g, buf);
  }
  int64_t score = 0;
  if (a < n) {
    // delta behind site a - 1 (unused when site a is a head)
    sg::Vec<K> d;
#pragma unroll
    for (int k = 0; k < K; k++) d.v[k] = 0;
    if (!sg::site_head(x[0])) {                                // (site 0 of the table is a head: a workgroup behind it has a carry)
      const sg::Vec<K> c = carry[blockIdx.x];
      if (threadIdx.x == 0) {
        d = c;
      } else {
        const FwdAgg<K> &ex = buf[threadIdx.x - 1];
        sg::Mat<K> m = ex.m;
        if (ex.flag) {
#pragma unroll
          for (int k = 0; k < K; k++) d.v[k] = m.a[k];
        } else {
          sg::maxplus_vec<K>(c, m, d);
        }
      }
    }
    sg::Vec<K> e;
    sg::emission<K>(t, sg::site_m(x[0]), sg::site_u(x[0]), e);
    if (sg::site_head(x[0])) sg::first_step<K>(t, e, d);
    else sg::viterbi_step<K>(t, e, d);
    unsigned long long f = 0;
#pragma unroll
    for (int i = 0; i < SG_T; i++) {
      if (a + (uint32_t)i < n) {                               // d is delta at site a + i
        uint32_t fi;
        sg::emission<K>(t, sg::site_m(x[i + 1]), sg::site_u(x[i + 1]), e);
        if (sg::site_head(x[i + 1])) {                         // the chain ends here, the next one starts
          int64_t best;
          fi = sg::map_constant(sg::best_state<K>(d, &best));
          score += best;
          sg::first_step<K>(t, e, d);
        } else {
          fi = sg::viterbi_step<K>(t, e, d);
        }
        f |= (unsigned long long)fi << (8 * i);
      }
    }
    if (a + SG_T <= n) {
      *reinterpret_cast<unsigned long long *>(fmap + a) = f;
    } else {
      for (uint32_t i = 0; a + i < n; i++) fmap[a + i] = (uint8_t)(f >> (8 * i));
    }
  }
  if (score != 0) atomicAdd(&l_score, (unsigned long long)score);   // (the scan's barriers are behind the zeroing)
  __syncthreads();
  if (threadIdx.x == 0 && l_score != 0) atomicAdd(&sc->score, l_score);
}

// ---- backward ------------------------------------------------------------------------------------------------------------

// f_a o f_{a+1} o ... over the thread's sites, from its 8 bytes (a site outside the table: the identity)
__device__ __forceinline__ uint32_t bwd_thread_agg(unsigned long long f, uint32_t a, uint32_t n) {
  uint32_t g = sg::kIdentityMap;
#pragma unroll
  for (int i = SG_T - 1; i >= 0; i--)
    if (a + (uint32_t)i < n) g = sg::map_compose((uint32_t)(f >> (8 * i)) & 0xFFu, g);
  return g;
}

__device__ __forceinline__ unsigned long long sg_load_bytes(const uint8_t *__restrict__ p, uint32_t a, uint32_t n) {
  if (a + SG_T <= n) return *reinterpret_cast<const unsigned long long *>(p + a);
  unsigned long long f = 0;
  for (uint32_t i = 0; a + i < n; i++) f |= (unsigned long long)p[a + i] << (8 * i);
  return f;
}

// Inclusive scan of maps over the workgroup's threads, thread tid's element applied AFTER those of the threads behind it in
// scan order: `reverse` scans from the last thread down (a suffix scan).  On return buf[tid] holds thread tid's result.
__device__ __forceinline__ uint32_t map_wg_scan(uint32_t mine, uint32_t *buf, bool reverse) {
  const uint32_t tid = threadIdx.x, r = reverse ? (uint32_t)SG_WG - 1u - tid : tid;   // the thread's place in scan order
  buf[tid] = mine;
  __syncthreads();
#pragma unroll 1
  for (uint32_t d = 1; d < (uint32_t)SG_WG; d <<= 1) {
    uint32_t other = sg::kIdentityMap;
    if (r >= d) other = buf[reverse ? tid + d : tid - d];
    __syncthreads();
    if (r >= d) { mine = sg::map_compose(mine, other); buf[tid] = mine; }
    __syncthreads();
  }
  return mine;
}

__global__ __launch_bounds__(SG_WG) void k_sg_bwd_agg(const uint8_t *__restrict__ fmap, uint32_t n, uint8_t *__restrict__ blkmap) {
  __shared__ uint32_t buf[SG_WG];
  const uint32_t a = blockIdx.x * (uint32_t)SG_B + threadIdx.x * (uint32_t)SG_T;
  const uint32_t g = map_wg_scan(bwd_thread_agg(a < n ? sg_load_bytes(fmap, a, n) : 0ull, a, n), buf, true);
  if (threadIdx.x == 0) blkmap[blockIdx.x] = (uint8_t)g;
}

// one workgroup: blkin[b] = the composition of the workgroups' maps behind b (the identity behind the last)
__global__ __launch_bounds__(SG_WG) void k_sg_bwd_carry(const uint8_t *__restrict__ blkmap, uint32_t nblk, uint8_t *__restrict__ blkin) {
  __shared__ uint32_t buf[SG_WG];
  // scan order r = nblk - 1 - b: the thread's r in [lo, hi)
  const uint32_t chunk = (nblk + SG_WG - 1) / SG_WG, lo = threadIdx.x * chunk, hi = lo + chunk < nblk ? lo + chunk : nblk;
  uint32_t g = sg::kIdentityMap;
  for (uint32_t r = lo; r < hi; r++) g = sg::map_compose(blkmap[nblk - 1u - r], g);
  map_wg_scan(g, buf, false);
  uint32_t run = threadIdx.x > 0 ? buf[threadIdx.x - 1] : sg::kIdentityMap;
  for (uint32_t r = lo; r < hi; r++) {
    blkin[nblk - 1u - r] = (uint8_t)run;
    run = sg::map_compose(blkmap[nblk - 1u - r], run);
  }
}

__global__ __launch_bounds__(SG_WG) void k_sg_bwd_walk(const uint8_t *__restrict__ fmap, uint32_t n, const uint8_t *__restrict__ blkin,
                                                       uint8_t *__restrict__ sstate) {
  __shared__ uint32_t buf[SG_WG];
  const uint32_t a = blockIdx.x * (uint32_t)SG_B + threadIdx.x * (uint32_t)SG_T;
  const unsigned long long f = a < n ? sg_load_bytes(fmap, a, n) : 0ull;
  map_wg_scan(bwd_thread_agg(f, a, n), buf, true);
  if (a >= n) return;                                          // (no barrier behind this line)
  const uint32_t behind = threadIdx.x + 1 < (uint32_t)SG_WG ? buf[threadIdx.x + 1] : sg::kIdentityMap;
  // every suffix holds a chain's end and is constant: any argument gives the state behind the thread's last site
  uint32_t st = sg::map_apply(sg::map_compose(behind, (uint32_t)blkin[blockIdx.x]), 0u);
  unsigned long long out = 0;
#pragma unroll
  for (int i = SG_T - 1; i >= 0; i--) {
    if (a + (uint32_t)i < n) {
      st = sg::map_apply((uint32_t)(f >> (8 * i)) & 0xFFu, st);
      out |= (unsigned long long)st << (8 * i);
    }
  }
  if (a + SG_T <= n) {
    *reinterpret_cast<unsigned long long *>(sstate + a) = out;
  } else {
    for (uint32_t i = 0; a + i < n; i++) sstate[a + i] = (uint8_t)(out >> (8 * i));
  }
}

// ---- refit counts, segments ----------------------------------------------------------------------------------------------

// a thread per site; every counter is a sum over the wave first (DPP), then one LDS add per wave, one global add per workgroup
template <int K>
__global__ __launch_bounds__(SG_WG) void k_sg_counts(const uint32_t *__restrict__ w, const uint8_t *__restrict__ sstate, uint32_t n,
                                                     SgScalars *__restrict__ sc) {
  __shared__ uint32_t l_cnt[28];
  if (threadIdx.x < 28) l_cnt[threadIdx.x] = 0;
  __syncthreads();
  const bool first = (threadIdx.x & 63) == 0;
  for (uint32_t base = blockIdx.x * (uint32_t)SG_WG; base < n; base += gridDim.x * (uint32_t)SG_WG) {   // (uniform over the workgroup)
    const uint32_t s = base + threadIdx.x;
    uint32_t st = 0xFFu, prev = 0xFFu, m = 0, u = 0, head = 0;  // (a thread without a site counts nothing)
    if (s < n) {
      const uint32_t x = w[s];
      st = sstate[s]; m = (uint32_t)sg::site_m(x); u = (uint32_t)sg::site_u(x); head = sg::site_head(x) ? 1u : 0u;
      if (!head) prev = sstate[s - 1];
    }
#pragma unroll
    for (int k = 0; k < K; k++) {                              // (every lane of the wave is here)
      const bool mine = st == (uint32_t)k;
      const uint32_t wm = wave_sum_u32(mine ? m : 0u), wu = wave_sum_u32(mine ? u : 0u), ws = wave_sum_u32(mine ? head : 0u);
      if (first && wm) atomicAdd(&l_cnt[k], wm);
      if (first && wu) atomicAdd(&l_cnt[K + k], wu);
      if (first && ws) atomicAdd(&l_cnt[2 * K + K * K + k], ws);
#pragma unroll
      for (int j = 0; j < K; j++) {
        const uint32_t wn = wave_sum_u32(mine && prev == (uint32_t)j ? 1u : 0u);
        if (first && wn) atomicAdd(&l_cnt[2 * K + j * K + k], wn);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)sg::count_words(K) && l_cnt[threadIdx.x]) atomicAdd(&sc->counts[threadIdx.x], (unsigned long long)l_cnt[threadIdx.x]);
}

__global__ __launch_bounds__(SG_WG) void k_sg_runs(const uint32_t *__restrict__ w, const uint8_t *__restrict__ sstate, uint32_t n,
                                                   uint32_t *__restrict__ flag) {
  const uint32_t s = blockIdx.x * (uint32_t)SG_WG + threadIdx.x;
  if (s >= n) return;
  flag[s] = sg::site_head(w[s]) || sstate[s] != sstate[s - 1] ? 1u : 0u;      // (site 0 is a head)
}

struct SgOut { int32_t *state; int32_t *icol[7]; double *dcol[3]; uint32_t nseg; };

// The rows of the segment table in three steps, no thread walking a whole run.  A site's segment is off[s] + flag[s] - 1 (site 0
// is flagged), and the segments are numbered in series order.
// (1) a thread per site: the state to the row order; a run's first site writes the row's keys, start and state, its last the end
__global__ __launch_bounds__(SG_WG) void k_sg_emit_sites(CxTab t, const uint32_t *__restrict__ ord, const uint8_t *__restrict__ sstate,
                                                         const uint32_t *__restrict__ flag, const uint32_t *__restrict__ off, SgOut o) {
  const uint32_t s = blockIdx.x * (uint32_t)SG_WG + threadIdx.x;
  if (s >= t.n) return;
  const uint32_t row = ord[s], f = flag[s], r = off[s] + f - 1u;
  const int32_t st = sstate[s];
  o.state[row] = st;
  if (r >= o.nseg) return;
  const bool last = s + 1 == t.n || flag[s + 1] != 0;
  if (f) {
    o.icol[0][r] = t.rname[row]; o.icol[1][r] = t.strand[row]; o.icol[2][r] = t.context[row]; o.icol[3][r] = t.pos[row]; o.icol[5][r] = st;
  }
  if (last) o.icol[4][r] = t.pos[row];
}

// (2) a thread per SG_T sites: the raw counts and the sites of the runs it crosses, one integer atomic add per run and thread into
// the row's meth and unmeth (as int64 in the double columns' memory, zeroed before) and nsites: exact, so the order does not matter
__global__ __launch_bounds__(SG_WG) void k_sg_emit_sums(CxTab t, const uint32_t *__restrict__ ord, const uint32_t *__restrict__ flag,
                                                        const uint32_t *__restrict__ off, SgOut o) {
  const uint32_t a = (blockIdx.x * (uint32_t)SG_WG + threadIdx.x) * (uint32_t)SG_T;
  if (a >= t.n) return;
  unsigned long long *meth = reinterpret_cast<unsigned long long *>(o.dcol[0]), *unmeth = reinterpret_cast<unsigned long long *>(o.dcol[1]);
  uint32_t r = off[a] + flag[a] - 1u;
  unsigned long long m = 0, u = 0;
  int32_t c = 0;
  for (uint32_t i = 0; i < (uint32_t)SG_T && a + i < t.n; i++) {
    if (i > 0 && flag[a + i]) {
      if (r < o.nseg) { atomicAdd(&meth[r], m); atomicAdd(&unmeth[r], u); atomicAdd(&o.icol[6][r], c); }
      r++; m = 0; u = 0; c = 0;
    }
    const uint32_t row = ord[a + i];
    m += (unsigned long long)t.meth[row]; u += (unsigned long long)t.unmeth[row]; c++;
  }
  if (r < o.nseg) { atomicAdd(&meth[r], m); atomicAdd(&unmeth[r], u); atomicAdd(&o.icol[6][r], c); }
}

// (3) a thread per row: the integer sums become the doubles (exact: they are below 2^53), and beta
__global__ __launch_bounds__(SG_WG) void k_sg_emit_rows(SgOut o) {
  const uint32_t r = blockIdx.x * (uint32_t)SG_WG + threadIdx.x;
  if (r >= o.nseg) return;
  const int64_t m = reinterpret_cast<const int64_t *>(o.dcol[0])[r], u = reinterpret_cast<const int64_t *>(o.dcol[1])[r];
  o.dcol[0][r] = (double)m; o.dcol[1][r] = (double)u; o.dcol[2][r] = (double)m / (double)(m + u);
}

// ---- host ----------------------------------------------------------------------------------------------------------------

static int64_t sg_blocks(int64_t n) { return (n + SG_B - 1) / SG_B; }

// The call's scratch, which epi_cx_segment_scratch_bytes states: the sort's workspace; the scalars (64-bit atomics); the site words
// (read 16 bytes at a time), f bytes and states (8 at a time); the workgroups' aggregates, carries (64-bit), maps; the scan's block sums
struct SgLayout : ScratchArena {
  size_t sort, scal, w, fmap, sstate, blkagg, carry, blkmap, blkin, scan;
  SgLayout(int64_t n, int K) {
    const size_t nblk = (size_t)sg_blocks(n);
    sort = reserve(SortPairs::bytes((size_t)n), 16); scal = reserve(sizeof(SgScalars));
    w = reserve((size_t)n * 4, 16); fmap = reserve((size_t)n, 16); sstate = reserve((size_t)n, 16);
    blkagg = reserve(nblk * (size_t)(8 * K * K + 8)); carry = reserve(nblk * (size_t)(8 * K));
    blkmap = reserve(nblk, 16); blkin = reserve(nblk, 16); scan = reserve(scan_tmp_bytes(n));
  }
};

struct SgBufs {
  const uint32_t *w; uint8_t *fmap, *sstate; uint64_t *blkagg, *carry; uint8_t *blkmap, *blkin; SgScalars *sc;   // (blkagg, carry: FwdAgg<K>, Vec<K>)
  uint32_t n, nblk;
};

// one decode: the forward and the backward scan, three launches each
template <int K> static void sg_decode(const SgBufs &b, const sg::Tables &t, hipStream_t s) {
  static_assert(sizeof(FwdAgg<K>) == 8 * K * K + 8 && sizeof(sg::Vec<K>) == 8 * K, "the layout's element sizes");
  FwdAgg<K> *blkagg = reinterpret_cast<FwdAgg<K> *>(b.blkagg);
  sg::Vec<K> *carry = reinterpret_cast<sg::Vec<K> *>(b.carry);
  prof_begin("segment_fwd_agg", s);
  hipLaunchKernelGGL(k_sg_fwd_agg<K>, dim3(b.nblk), dim3(SG_WG), 0, s, b.w, b.n, t, blkagg);
  prof_end("segment_fwd_agg", s);
  prof_begin("segment_fwd_carry", s);
  hipLaunchKernelGGL(k_sg_fwd_carry<K>, dim3(1), dim3(SG_WG), 0, s, blkagg, b.nblk, carry);
  prof_end("segment_fwd_carry", s);
  prof_begin("segment_fwd_walk", s);
  hipLaunchKernelGGL(k_sg_fwd_walk<K>, dim3(b.nblk), dim3(SG_WG), 0, s, b.w, b.n, t, carry, b.fmap, b.sc);
  prof_end("segment_fwd_walk", s);
  prof_begin("segment_bwd_agg", s);
  hipLaunchKernelGGL(k_sg_bwd_agg, dim3(b.nblk), dim3(SG_WG), 0, s, b.fmap, b.n, b.blkmap);
  prof_end("segment_bwd_agg", s);
  prof_begin("segment_bwd_carry", s);
  hipLaunchKernelGGL(k_sg_bwd_carry, dim3(1), dim3(SG_WG), 0, s, b.blkmap, b.nblk, b.blkin);
  prof_end("segment_bwd_carry", s);
  prof_begin("segment_bwd_walk", s);
  hipLaunchKernelGGL(k_sg_bwd_walk, dim3(b.nblk), dim3(SG_WG), 0, s, b.fmap, b.n, b.blkin, b.sstate);
  prof_end("segment_bwd_walk", s);
}

static void sg_tables(int K, const int32_t *words, sg::Tables &t) {
  t = sg::Tables();
  if (K == 2) sg::tables_unpack<2>(words, t); else if (K == 3) sg::tables_unpack<3>(words, t); else sg::tables_unpack<4>(words, t);
}

struct SgCall {
  int32_t K, max_gap, max_coverage, max_iter;
  int32_t *d_state; int32_t *const *seg_i; double *const *seg_d; int64_t seg_cap;
};

static int cx_segment(epi_engine *e, const CxTab &t, const SgCall &c, epi_segment_fit &fit, hipStream_t s, int64_t *nchain_out,
                      int64_t *nsegment_out) {
  const char *who = "epi_cx_segment_dev";
  const int K = c.K;
  const int64_t n = t.n, nsite_blk = (n + SG_WG - 1) / SG_WG;
  EPI_TRY(check_grid(nsite_blk, SG_WG, "segmentation kernels"));
  SgLayout lay(n, K);                                         // (goes when the call returns)
  EPI_TRY(lay.alloc());
  uint64_t *sort_mem; uint32_t *w, *scan; SgScalars *sc; SgBufs b;
  EPI_TRY(lay.at(lay.sort, &sort_mem)); EPI_TRY(lay.at(lay.scal, &sc)); EPI_TRY(lay.at(lay.w, &w, 16)); EPI_TRY(lay.at(lay.fmap, &b.fmap, 8));
  EPI_TRY(lay.at(lay.sstate, &b.sstate, 8)); EPI_TRY(lay.at(lay.blkagg, &b.blkagg)); EPI_TRY(lay.at(lay.carry, &b.carry));
  EPI_TRY(lay.at(lay.blkmap, &b.blkmap)); EPI_TRY(lay.at(lay.blkin, &b.blkin)); EPI_TRY(lay.at(lay.scan, &scan));
  SortPairs sort(sort_mem, (size_t)n);
  DevBuf scan_tmp = DevBuf::view(scan, scan_tmp_bytes(n));
  b.w = w; b.sc = sc; b.n = (uint32_t)n; b.nblk = (uint32_t)sg_blocks(n);
  EPI_HIP(hipMemsetAsync(sc, 0, sizeof(SgScalars), s));

  EPI_TRY(series_sort(t, sort, &sc->unsorted, &sc->bad, scan_tmp, "segment_sort", s));
  const uint32_t *ord = sort.vals();
  prof_begin("segment_gather", s);
  hipLaunchKernelGGL(k_sg_gather, dim3((unsigned)nsite_blk), dim3(SG_WG), 0, s, t, sort.keys(), ord, c.max_gap, c.max_coverage, w, sc);
  prof_end("segment_gather", s);
  EPI_HIP(hipGetLastError());

  SgScalars h;                                                // the input's verdict, before any decode
  EPI_TRY(read_scalars(e, s, sc, sizeof(h), &h));
  EPI_TRY(series_verdict(who, h.unsorted, h.bad));
  const int64_t nchain = h.nchain;

  int32_t words[28], next_words[28];
  const int nw = sg::table_words(K);
  sg::quantise_tables(K, fit.p, fit.trans, fit.init, words);
  int32_t iterations = 0, converged = 0;
  for (int32_t it = 1; it <= c.max_iter; it++) {
    sg::Tables tab;
    sg_tables(K, words, tab);
    EPI_HIP(hipMemsetAsync(&sc->score, 0, sizeof(SgScalars) - offsetof(SgScalars, score), s));
    if (K == 2) sg_decode<2>(b, tab, s); else if (K == 3) sg_decode<3>(b, tab, s); else sg_decode<4>(b, tab, s);
    EPI_HIP(hipGetLastError());
    iterations = it;
    if (it == c.max_iter) break;
    prof_begin("segment_counts", s);
    // at most SG_COUNT_WGS workgroups, each over a strided share of the sites: every workgroup ends with one atomic per counter on
    // the same few addresses, which a workgroup per 256 sites made the whole cost of the kernel
    const unsigned cgrid = (unsigned)(nsite_blk < SG_COUNT_WGS ? nsite_blk : SG_COUNT_WGS);
    if (K == 2) hipLaunchKernelGGL(k_sg_counts<2>, dim3(cgrid), dim3(SG_WG), 0, s, b.w, b.sstate, b.n, sc);
    else if (K == 3) hipLaunchKernelGGL(k_sg_counts<3>, dim3(cgrid), dim3(SG_WG), 0, s, b.w, b.sstate, b.n, sc);
    else hipLaunchKernelGGL(k_sg_counts<4>, dim3(cgrid), dim3(SG_WG), 0, s, b.w, b.sstate, b.n, sc);
    prof_end("segment_counts", s);
    EPI_HIP(hipGetLastError());
    EPI_TRY(read_scalars(e, s, sc, sizeof(h), &h));           // the counters, once per iteration
    int64_t counts[28];
    for (int x = 0; x < nw; x++) counts[x] = (int64_t)h.counts[x];
    double p[4], trans[16], init[4];
    for (int k = 0; k < K; k++) { p[k] = fit.p[k]; init[k] = fit.init[k]; }
    for (int x = 0; x < K * K; x++) trans[x] = fit.trans[x];
    sg::reestimate(K, counts, p, trans, init);
    sg::quantise_tables(K, p, trans, init, next_words);
    bool same = true;
    for (int x = 0; x < nw; x++) same = same && next_words[x] == words[x];
    if (same) { converged = 1; break; }                       // (the parameters reported are those of the last decode)
    for (int k = 0; k < K; k++) { fit.p[k] = p[k]; fit.init[k] = init[k]; }
    for (int x = 0; x < K * K; x++) fit.trans[x] = trans[x];
    for (int x = 0; x < nw; x++) words[x] = next_words[x];
  }

  uint32_t *flag = sort.spare<uint32_t>(), *off = flag + n;
  prof_begin("segment_runs", s);
  hipLaunchKernelGGL(k_sg_runs, dim3((unsigned)nsite_blk), dim3(SG_WG), 0, s, b.w, b.sstate, b.n, flag);
  const int rc_scan = scan_exclusive_u32(flag, off, n, &sc->nsegment, scan_tmp, s);
  prof_end("segment_runs", s);
  EPI_HIP(hipGetLastError());
  EPI_TRY(rc_scan);
  EPI_TRY(read_scalars(e, s, sc, sizeof(h), &h));             // the last synchronisation before anything is written
  *nsegment_out = h.nsegment;                                 // (the count needed, when the refusal below is the answer)
  EPI_TRY(cx_rows_fit(who, "rows", h.nsegment, c.seg_cap));
  SgOut o;
  o.state = c.d_state;
  for (int i = 0; i < 7; i++) o.icol[i] = c.seg_i[i];
  for (int i = 0; i < 3; i++) o.dcol[i] = c.seg_d[i];
  o.nseg = h.nsegment;
  prof_begin("segment_emit", s);
  EPI_HIP(hipMemsetAsync(o.dcol[0], 0, (size_t)h.nsegment * 8, s));
  EPI_HIP(hipMemsetAsync(o.dcol[1], 0, (size_t)h.nsegment * 8, s));
  EPI_HIP(hipMemsetAsync(o.icol[6], 0, (size_t)h.nsegment * 4, s));
  hipLaunchKernelGGL(k_sg_emit_sites, dim3((unsigned)nsite_blk), dim3(SG_WG), 0, s, t, ord, b.sstate, flag, off, o);
  hipLaunchKernelGGL(k_sg_emit_sums, dim3(b.nblk), dim3(SG_WG), 0, s, t, ord, flag, off, o);
  hipLaunchKernelGGL(k_sg_emit_rows, dim3((h.nsegment + SG_WG - 1) / SG_WG), dim3(SG_WG), 0, s, o);
  prof_end("segment_emit", s);
  EPI_HIP(hipGetLastError());
  EPI_HIP(hipStreamSynchronize(s));                           // (the scratch goes back when this returns)
  fit.iterations = iterations; fit.converged = converged; fit.score = (int64_t)h.score;
  *nchain_out = nchain;
  return EPI_OK;
}

}  // namespace epi

using namespace epi;

extern "C" {

int epi_segment_block_sites(void) { return SG_B; }
int epi_segment_thread_sites(void) { return SG_T; }

int epi_cx_segment_scratch_bytes(int64_t n, int32_t nstates, int64_t *bytes_out) {
  const char *who = "epi_cx_segment_scratch_bytes";
  if (!bytes_out) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  *bytes_out = 0;
  if (nstates < EPI_SEGMENT_MIN_STATES || nstates > EPI_SEGMENT_MAX_STATES)
    return fail(EPI_ERR_ARG, "%s: nstates = %d, from %d to %d", who, nstates, EPI_SEGMENT_MIN_STATES, EPI_SEGMENT_MAX_STATES);
  EPI_TRY(cx_rows_arg(who, n, {EPI_SEGMENT_MAX_SITES, "2^26"}));
  if (n > 0) *bytes_out = (int64_t)SgLayout(n, nstates).used;
  return EPI_OK;
}

int epi_cx_segment_dev(epi_engine *e, const int32_t *const d_in[6], int64_t n, int32_t nstates, const double *p, const double *trans,
                       const double *init, int32_t max_gap, int32_t max_coverage, int32_t max_iter, int32_t *d_state, int32_t *const d_seg_i[7],
                       double *const d_seg_d[3], int64_t seg_cap, void *stream, epi_segment_fit *fit_out, int64_t *nchain_out,
                       int64_t *nsegment_out) {
  const char *who = "epi_cx_segment_dev";
  if (!fit_out || !nchain_out || !nsegment_out) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  EPI_TRY(sg::check_model(who, nstates, p, trans, init));
  if (max_gap < 0) return fail(EPI_ERR_ARG, "%s: negative max_gap", who);
  if (max_coverage < 1 || max_coverage > EPI_SEGMENT_MAX_COVERAGE)
    return fail(EPI_ERR_ARG, "%s: max_coverage = %d, from 1 to %d", who, max_coverage, EPI_SEGMENT_MAX_COVERAGE);
  if (max_iter < 1) return fail(EPI_ERR_ARG, "%s: max_iter = %d, at least 1", who, max_iter);
  CxTab t;
  EPI_TRY(cx_tab_arg(who, d_in, n, {EPI_SEGMENT_MAX_SITES, "2^26"}, &t, seg_cap));
  if (!e) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  epi_segment_fit fit = {};
  fit.nstates = nstates;
  for (int k = 0; k < nstates; k++) { fit.p[k] = p[k]; fit.init[k] = init[k]; }
  for (int x = 0; x < nstates * nstates; x++) fit.trans[x] = trans[x];
  if (n == 0) { *fit_out = fit; *nchain_out = 0; *nsegment_out = 0; return EPI_OK; }
  if (!d_state) return fail(EPI_ERR_ARG, "%s: NULL argument", who);
  EPI_TRY(cx_cols_arg(who, d_seg_i, 7, d_seg_d, 3));
  EPI_HIP(hipSetDevice(e->device));
  SgCall c = {nstates, max_gap, max_coverage, max_iter, d_state, d_seg_i, d_seg_d, seg_cap};
  int64_t nchain = 0;
  EPI_TRY(cx_segment(e, t, c, fit, reinterpret_cast<hipStream_t>(stream), &nchain, nsegment_out));
  *fit_out = fit; *nchain_out = nchain;
  return EPI_OK;
}

}  // extern "C"
