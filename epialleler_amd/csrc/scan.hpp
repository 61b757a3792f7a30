// Scans, at three levels: over the 64 lanes of a wave, over one value per thread of a workgroup, and over a device array in
// three launches.  Device code only (common.hpp includes this file for the .hip units).  DESIGN.md 4.22 lists the users and the
// scans that stay apart.
//
// An operator is a struct with `using T`, `identity()` and `combine(a, b)`, where a stands in front of b.  `dpp` picks the
// wave ladder; `invertible` operators also have `remove(inclusive, v)`, which takes a thread's own value out again.
#pragma once
#include "common.hpp"

namespace epi {

template <class U, bool DPP> struct ScanSum {
  using T = U;
  static constexpr bool dpp = DPP, invertible = true;
  static __host__ __device__ __forceinline__ T identity() { return 0; }
  static __device__ __forceinline__ T combine(T a, T b) { return a + b; }
  static __device__ __forceinline__ T remove(T inc, T v) { return inc - v; }
};
using SumU32 = ScanSum<uint32_t, true>;
using SumU64 = ScanSum<unsigned long long, false>;   // (its sites were written on the shuffle ladder and stay there)
template <bool MAX> struct MinMaxF64 {               // exact and order-free as long as no NaN and no -0.0 comes in
  using T = double;
  static constexpr bool dpp = false, invertible = false;
  static __host__ __device__ __forceinline__ T identity() { return MAX ? -__builtin_inf() : __builtin_inf(); }
  static __device__ __forceinline__ T combine(T a, T b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); }
};

// ---- wave ----------------------------------------------------------------------------------------------------------------
// Inclusive prefix sum over the 64 lanes as DPP moves (row_shr 1, 2, 4, 8 inside a row of 16 lanes, then row_bcast:15 into
// rows 1 and 3 and row_bcast:31 into rows 2 and 3): VALU instructions, where __shfl_* is a ds_bpermute through the LDS pipe
// with ~100 cycles of latency.
// (bound_ctrl = true on the row shifts: a lane without a source reads 0, the same value as `old` = 0 would give it, and the
//  compiler can then fold move and add into one v_add_u32_dpp instead of v_mov 0 + v_mov_dpp + v_add)
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t scan_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWS, 0xF, ROWS == 0xF);   // lanes without a source get 0
}
template <int CTRL, int ROWS>
__device__ __forceinline__ unsigned long long scan_dpp(unsigned long long v) {
  return ((unsigned long long)scan_dpp<CTRL, ROWS>((uint32_t)(v >> 32)) << 32) | scan_dpp<CTRL, ROWS>((uint32_t)v);
}
template <class ST>
__device__ __forceinline__ ST wave_scan_dpp(ST v) {
  v += scan_dpp<0x111, 0xF>(v);
  v += scan_dpp<0x112, 0xF>(v);
  v += scan_dpp<0x114, 0xF>(v);
  v += scan_dpp<0x118, 0xF>(v);
  v += scan_dpp<0x142, 0xA>(v);
  v += scan_dpp<0x143, 0xC>(v);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {       // sum over the 64 lanes (uniform result)
  return (uint32_t)__builtin_amdgcn_readlane((int)wave_scan_dpp(v), 63);
}

template <class Op>
__device__ __forceinline__ typename Op::T wave_scan(typename Op::T v) {   // inclusive over the 64 lanes
  if constexpr (Op::dpp) return wave_scan_dpp(v);
  else {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const typename Op::T o = __shfl_up(v, d, 64);
      if (lane >= d) v = Op::combine(o, v);
    }
    return v;
  }
}

// ---- workgroup -------------------------------------------------------------------------------------------------------------
// One value per thread of a workgroup of WG threads: wave scan, lane 63 parks the wave's total in s_wave [WG / 64], and behind
// one barrier every thread combines the totals of the waves in front of it; *total (when asked for) = the workgroup's
// aggregate.  REUSE puts a second barrier in front: a caller that comes back with the same s_wave in a loop needs it (a wave
// may still be reading the last round's totals).
template <class Op, int WG, bool REUSE, bool EXCLUSIVE>
__device__ __forceinline__ typename Op::T wg_scan_any(typename Op::T v, typename Op::T *s_wave, typename Op::T *total) {
  using T = typename Op::T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T inc = wave_scan<Op>(v);
  T mine = inc;
  if constexpr (EXCLUSIVE) {
    // without an inverse: the inclusive value of the lane before (lane 0: nothing of this wave lies in front)
    if constexpr (Op::invertible) mine = Op::remove(inc, v);
    else { mine = __shfl_up(inc, 1, 64); if (lane == 0) mine = Op::identity(); }
  }
  if constexpr (REUSE) __syncthreads();
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  T before = Op::identity(), all = Op::identity();
#pragma unroll
  for (int w = 0; w < WG / 64; w++) {
    const T x = s_wave[w];
    if (w < wave) before = Op::combine(before, x);
    all = Op::combine(all, x);
  }
  if (total) *total = all;
  return Op::combine(before, mine);
}
template <class Op, int WG, bool REUSE = false>
__device__ __forceinline__ typename Op::T wg_scan(typename Op::T v, typename Op::T *s_wave, typename Op::T *total = nullptr) {
  return wg_scan_any<Op, WG, REUSE, false>(v, s_wave, total);
}
template <class Op, int WG, bool REUSE = false>
__device__ __forceinline__ typename Op::T wg_scan_excl(typename Op::T v, typename Op::T *s_wave, typename Op::T *total = nullptr) {
  return wg_scan_any<Op, WG, REUSE, true>(v, s_wave, total);
}
// the inclusive values as a table to search in: s[t + 1] for thread t, s[0] = the identity (s [WG + 1]); published by a barrier,
// which also makes s_wave free for the next call
template <class Op, int WG>
__device__ __forceinline__ void wg_scan_table(typename Op::T v, typename Op::T *s, typename Op::T *s_wave) {
  s[threadIdx.x + 1] = wg_scan<Op, WG>(v, s_wave);
  if (threadIdx.x == 0) s[0] = Op::identity();
  __syncthreads();
}

// ---- device ----------------------------------------------------------------------------------------------------------------
// Scan of n elements in three launches, reduce-then-scan: a workgroup owns ITEMS * WG consecutive elements, a thread ITEMS
// consecutive ones.  k_scan_reduce leaves each workgroup's aggregate in agg; k_scan_carry (ONE workgroup, WG aggregates per
// round) replaces agg[k] by everything in front of workgroup k, starting from `seed`, and stores the grand total; k_scan_apply
// loads the elements again and hands each to store(i, exclusive, inclusive).  No kernel waits on another workgroup.  load(i)
// and store(...) are functor structs passed by value; an element is loaded and stored by the same thread, so a scan in place
// is fine.  The operators above are exact, so no launch shape enters a result.
template <class Op, int ITEMS, int WG, class Load>
__global__ __launch_bounds__(WG) void k_scan_reduce(int64_t n, Load load, typename Op::T *__restrict__ agg) {
  using T = typename Op::T;
  __shared__ T s_wave[WG / 64];
  const int64_t base = (int64_t)blockIdx.x * (ITEMS * WG) + (int64_t)threadIdx.x * ITEMS;
  T acc = Op::identity();
#pragma unroll
  for (int i = 0; i < ITEMS; i++) if (base + i < n) acc = Op::combine(acc, load(base + i));
  T total;
  (void)wg_scan<Op, WG>(acc, s_wave, &total);
  if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

template <class Op, int WG>
__global__ __launch_bounds__(WG) void k_scan_carry(typename Op::T *__restrict__ agg, int64_t nb, typename Op::T seed,
                                                   typename Op::T *__restrict__ d_total) {
  using T = typename Op::T;
  __shared__ T s_wave[WG / 64];
  T carry = seed;
  for (int64_t base = 0; base < nb; base += WG) {
    const int64_t k = base + threadIdx.x;
    const T v = k < nb ? agg[k] : Op::identity();
    T total;
    const T ex = wg_scan_excl<Op, WG, true>(v, s_wave, &total);
    if (k < nb) agg[k] = Op::combine(carry, ex);
    carry = Op::combine(carry, total);
  }
  if (threadIdx.x == 0 && d_total) *d_total = carry;
}

template <class Op, int ITEMS, int WG, class Load, class Store>
__global__ __launch_bounds__(WG) void k_scan_apply(int64_t n, Load load, Store store, const typename Op::T *__restrict__ agg) {
  using T = typename Op::T;
  __shared__ T s_wave[WG / 64];
  const int64_t base = (int64_t)blockIdx.x * (ITEMS * WG) + (int64_t)threadIdx.x * ITEMS;
  T v[ITEMS];
  T acc = Op::identity();
#pragma unroll
  for (int i = 0; i < ITEMS; i++) {
    v[i] = base + i < n ? load(base + i) : Op::identity();
    acc = Op::combine(acc, v[i]);
  }
  T ex = Op::combine(agg[blockIdx.x], wg_scan_excl<Op, WG>(acc, s_wave));
#pragma unroll
  for (int i = 0; i < ITEMS; i++) {
    const T inc = Op::combine(ex, v[i]);
    if (base + i < n) store(base + i, ex, inc);
    ex = inc;
  }
}

// the carry launch alone: agg [nb] -> its exclusive scan in place
template <class Op, int WG>
int device_scan_carry(typename Op::T *agg, int64_t nb, typename Op::T seed, typename Op::T *d_total, hipStream_t s) {
  hipLaunchKernelGGL((k_scan_carry<Op, WG>), dim3(1), dim3(WG), 0, s, agg, nb, seed, d_total);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

// n > 0; d_total may be NULL; tmp: a word of T per workgroup
template <class Op, int ITEMS, int WG, class Load, class Store>
int device_scan(int64_t n, Load load, Store store, typename Op::T seed, typename Op::T *d_total, DevBuf &tmp, hipStream_t s) {
  using T = typename Op::T;
  const int64_t nb = (n + ITEMS * WG - 1) / (ITEMS * WG);
  EPI_TRY(tmp.ensure((size_t)nb * sizeof(T)));
  T *agg = tmp.as<T>();
  hipLaunchKernelGGL((k_scan_reduce<Op, ITEMS, WG, Load>), dim3((unsigned)nb), dim3(WG), 0, s, n, load, agg);
  EPI_TRY((device_scan_carry<Op, WG>(agg, nb, seed, d_total, s)));
  hipLaunchKernelGGL((k_scan_apply<Op, ITEMS, WG, Load, Store>), dim3((unsigned)nb), dim3(WG), 0, s, n, load, store, agg);
  EPI_HIP(hipGetLastError());
  return EPI_OK;
}

}  // namespace epi
