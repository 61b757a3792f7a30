// One record's CIGAR walked by one wavefront, query base by query base (device code only).  Shared by callMethylation's
// k_call_refspace (call_methylation.hip) and the template assembly of preprocessBam(mates = "anywhere")
// (assemble_templates.hip).
//
// The ops are taken 64 at a time: their query and reference lengths are scanned across the lanes (DPP), the prefixes
// go to LDS, and each lane finds the op of its query position by a 6-step search over them.  f(q, op, r) is called
// once for every query base q < l_seq that an op consumes (M I S = X), with r the reference offset (from the record's
// first aligned base) of that base: the op's reference start plus q's offset inside the op.  Within one record no two
// query bases of an M / = / X op share a reference offset.
#pragma once
#include "common.hpp"

namespace epi {

// LDS written by some lanes of the wave and read by others: keep the compiler's order and wait for the writes
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct CigarLds {            // one wave's prefixes of a group of 64 ops
  uint32_t qe[64];           // query end of op k (inclusive prefix of the query lengths)
  uint32_t rs[64];           // reference start of op k (exclusive prefix of the reference lengths)
  uint8_t op[64];
};

// returns the record's reference length (sum of the M D N = X lengths)
template <class F>
__device__ __forceinline__ uint32_t wave_cigar_walk(const uint32_t *__restrict__ cigar, int32_t n_cig, int32_t l_seq,
                                                    CigarLds &s, int lane, F &&f) {
  uint32_t qcarry = 0, rcarry = 0;
  for (int32_t o0 = 0; o0 < n_cig; o0 += 64) {
    const int32_t o = o0 + lane;
    uint32_t op = 9, len = 0;                           // (lanes past the last op: 'B', which consumes nothing)
    if (o < n_cig) { const uint32_t v = cigar[o]; op = v & 15; len = v >> 4; }
    const uint32_t ql = (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) ? len : 0;
    const uint32_t rl = (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ? len : 0;
    const uint32_t qe = qcarry + wave_scan_dpp(ql), re = rcarry + wave_scan_dpp(rl);
    s.qe[lane] = qe;
    s.rs[lane] = re - rl;
    s.op[lane] = (uint8_t)op;
    wave_lds_sync();
    const uint32_t qend = (uint32_t)__builtin_amdgcn_readlane((int)qe, 63);
    for (uint32_t q0 = qcarry; q0 < qend; q0 += 64) {
      const uint32_t q = q0 + lane;
      if (q < qend && q < (uint32_t)l_seq) {
        int k = 0;                                      // ops of this group that end at or before q
#pragma unroll
        for (int st = 32; st > 0; st >>= 1) k += s.qe[k + st - 1] <= q ? st : 0;
        const uint32_t qs = k > 0 ? s.qe[k - 1] : qcarry;
        f(q, (uint32_t)s.op[k], s.rs[k] + (q - qs));
      }
    }
    qcarry = qend;
    rcarry = (uint32_t)__builtin_amdgcn_readlane((int)re, 63);
    wave_lds_sync();                                    // (the next group overwrites the prefixes)
  }
  return rcarry;
}

}  // namespace epi
