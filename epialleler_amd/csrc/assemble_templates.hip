// preprocessBam(mates = "anywhere"): each template's merged row, built in its final output slot.
//
// The host (bam_pack.cpp; the uploads: bam_device.cpp) has paired the records through their QNAMEs, uploaded every kept
// record's CIGAR ops, packed query bytes (nt16 << 4) | ctx and QUAL to a device arena, and at the end of the file ordered
// each template's records (READ1 before READ2, ties in file order), computed its start, width and trims and sorted the rows.  What is left is the
// byte work of the reference's template merge (src/rcpp_read_bam.cpp:84-151, pack_pe in bam_pack.cpp):
//   every position starts at quality q0 and byte 0xFB; the records are applied in merge order, and a query base of an
//   M / = / X op replaces the position's byte when its quality is strictly higher than the position's (a tie keeps the
//   earlier record's byte).
//
// One wavefront per template (four per workgroup).  The row's qualities and bytes sit in LDS when the row is at most
// kAsmLdsWidth long, else in global memory (the output row itself and a quality scratch).  Only the kept part of the row
// [trim5, trim5 + keep) is tracked: a position outside it never reaches the output.  A record's query bases go 64 at a
// time over the lanes, each finding its CIGAR op by the prefix search of wave_cigar_walk (cigar_walk.hpp); within one
// record no two query bases land on the same position, so a record's writes cannot race, and the records of a template
// are ordered by the wave's program order with a wave-level barrier between them.
#include "common.hpp"
#include "cigar_walk.hpp"

#include <chrono>

namespace epi {
namespace {

constexpr int kWaves = 4;                           // templates per workgroup of 256 threads

// between two records: LDS rows need the wave's LDS order; global rows its memory order at workgroup scope (the L1 the
// wave's lanes share)
template <bool kLds>
__device__ __forceinline__ void row_sync() {
  if (kLds) {
    wave_lds_sync();
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
}

template <bool kLds>
__device__ __forceinline__ void merge_row(const AsmTpl &T, const AsmRec *__restrict__ recs, const uint8_t *__restrict__ arena,
                                          uint8_t q0, int32_t trim5, uint8_t *tq, uint8_t *tb, CigarLds &sc, int lane) {
  const int32_t keep = T.keep;
  for (int32_t j = lane; j < keep; j += 64) { tq[j] = q0; tb[j] = 0xFB; }
  row_sync<kLds>();
  for (int32_t k = 0; k < T.nrec; k++) {
    const AsmRec R = recs[T.rec_lo + k];
    const uint32_t *cig = reinterpret_cast<const uint32_t *>(arena + R.arena_off);
    const uint8_t *pb = arena + R.arena_off + 4 * (int64_t)R.n_cig, *ql = pb + R.l_seq;
    const int64_t base = (int64_t)R.dest0 - trim5;   // row position of the record's first aligned base
    wave_cigar_walk(cig, R.n_cig, R.l_seq, sc, lane, [&](uint32_t q, uint32_t op, uint32_t rq) {
      if (op == 0 || op == 7 || op == 8) {
        const int64_t j = base + rq;
        if (j >= 0 && j < keep) {
          const uint8_t qq = ql[q];
          if (qq > tq[j]) { tq[j] = qq; tb[j] = pb[q]; }
        }
      }
    });
    row_sync<kLds>();
  }
}

__global__ __launch_bounds__(256) void k_assemble_templates(const AsmTpl *__restrict__ tpl, int64_t ntpl,
                                                            const AsmRec *__restrict__ recs, const uint8_t *__restrict__ arena,
                                                            uint8_t q0, int32_t trim5, uint8_t *__restrict__ xm,
                                                            uint8_t *__restrict__ qscr) {
  __shared__ uint8_t s_q[kWaves][kAsmLdsWidth], s_b[kWaves][kAsmLdsWidth];
  __shared__ CigarLds s_cig[kWaves];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t t = (int64_t)blockIdx.x * kWaves + w;
  if (t >= ntpl) return;                             // (whole waves: no workgroup barrier below)
  const AsmTpl T = tpl[t];
  uint8_t *out = xm + T.out_off;
  if (T.keep <= kAsmLdsWidth) {
    merge_row<true>(T, recs, arena, q0, trim5, s_q[w], s_b[w], s_cig[w], lane);
    for (int32_t j = lane; j < T.keep; j += 64) out[j] = s_b[w][j];
  } else {
    merge_row<false>(T, recs, arena, q0, trim5, qscr + T.q_off, out, s_cig[w], lane);
  }
}

}  // namespace

int assemble_templates(epi_engine *eng, const uint8_t *d_arena, const AsmTpl *tpl, int64_t ntpl, const AsmRec *recs,
                       int64_t nrec, uint8_t q0, int32_t trim5, int64_t nbytes, int64_t qbytes, uint8_t *h_out,
                       double *t_kernel, double *t_d2h) {
  auto tnow = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  *t_kernel = *t_d2h = 0;
  if (ntpl <= 0 || nbytes <= 0) return EPI_OK;       // (no row has a byte)
  EPI_HIP(hipSetDevice(eng->device));
  hipStream_t s = eng->stream;
  const int64_t nblk = (ntpl + kWaves - 1) / kWaves;
  EPI_TRY(check_grid(nblk, 256, "preprocessBam"));
  DevBuf d_tpl, d_rec, d_out, d_q;
  EPI_TRY(d_tpl.ensure((size_t)ntpl * sizeof(AsmTpl)));
  EPI_TRY(d_rec.ensure((size_t)(nrec > 0 ? nrec : 1) * sizeof(AsmRec)));
  EPI_TRY(d_out.ensure((size_t)nbytes));
  if (qbytes > 0) EPI_TRY(d_q.ensure((size_t)qbytes));
  EPI_HIP(hipMemcpyAsync(d_tpl.p, tpl, (size_t)ntpl * sizeof(AsmTpl), hipMemcpyHostToDevice, s));
  if (nrec > 0) EPI_HIP(hipMemcpyAsync(d_rec.p, recs, (size_t)nrec * sizeof(AsmRec), hipMemcpyHostToDevice, s));
  EPI_HIP(hipStreamSynchronize(s));
  double t0 = tnow();
  prof_begin("assemble_templates", s);
  hipLaunchKernelGGL(k_assemble_templates, dim3((unsigned)nblk), dim3(256), 0, s, d_tpl.as<AsmTpl>(), ntpl, d_rec.as<AsmRec>(),
                     d_arena, q0, trim5, d_out.as<uint8_t>(), d_q.as<uint8_t>());
  EPI_HIP(hipGetLastError());
  prof_end("assemble_templates", s);
  EPI_HIP(hipStreamSynchronize(s));
  *t_kernel = tnow() - t0;
  t0 = tnow();
  EPI_TRY(copy_to_host(eng, h_out, d_out.p, (size_t)nbytes, s));
  EPI_HIP(hipStreamSynchronize(s));
  *t_d2h = tnow() - t0;
  return EPI_OK;
}

}  // namespace epi
