// callMethylation's per-base core (src/rcpp_call_methylation.cpp:102-165 restated): for every query base of a record,
// the reference base that the CIGAR puts under it, the cytosine context of the triad around it, and the call.
//
// Two kernels, one wavefront per record in both; the lanes span query positions, 64 at a time, so a read of several
// kilobases is spread over the wave like a short one:
//   k_call_refspace  the CIGAR, 64 ops at a time (wave_cigar_walk, cigar_walk.hpp): query and reference lengths are
//                    scanned across the lanes (DPP), the prefixes go to LDS, and each lane finds the op of its query
//                    position by a 6-step search over them.  M / = copy the genome base, X / I / S give N, D / N move the reference only, H / P / B do
//                    nothing.  Output: the record's reference in query space as 3-bit codes, with two bases of halo on
//                    each side (N beyond the contig), in a scratch array.
//   k_call_xm        per query base: the triad at offsets 0..2 (forward table, strand C/T) or -2..0 (reverse table,
//                    strand G/A) keys a 512-entry context table in LDS; a base with a context is upper case when the
//                    read shows the methylated base, '.' when it shows neither that nor the converted one, and lower
//                    case otherwise.  Two output forms of one kernel: the XM letter (callMethylation, BAM out) or the
//                    reader's packed template byte (nt16 << 4) | ctx_to_idx(XM) (preprocessBam with a genome), which is
//                    what bam_pack.cpp's packed_bytes() makes of SEQ and the XM letter.
// The kernel boundary orders the scratch writes of the first before the reads of the second.  The host (call_select in
// bam_call.cpp) has checked every record it hands over: the contig exists, the CIGAR consumes exactly l_seq query bases and the
// aligned span lies inside the contig; the kernels still keep every genome read inside its contig.
#include "common.hpp"
#include "cigar_walk.hpp"

namespace epi {
namespace {

constexpr int kWaves = 4;                           // records per workgroup of 256 threads

__device__ __forceinline__ bool tri_ok_dev(uint32_t c) { return c == 1 || c == 3 || c == 4 || c == 6 || c == 7; }
// the context tables of src/epialleleR.h:43-116, keyed by the low three bits of the three letters (A=1 C=3 T=4 N=6 G=7)
__device__ __forceinline__ uint8_t ctx_forward_dev(uint32_t b0, uint32_t b1, uint32_t b2) {   // C at i: CG z, CHG x, CHH h
  if (b0 != 3 || !tri_ok_dev(b1) || !tri_ok_dev(b2)) return '.';
  return b1 == 7 ? 'z' : b2 == 7 ? 'x' : 'h';
}
__device__ __forceinline__ uint8_t ctx_reverse_dev(uint32_t b0, uint32_t b1, uint32_t b2) {   // G at i (i-2, i-1, i)
  if (b2 != 7 || !tri_ok_dev(b0) || !tri_ok_dev(b1)) return '.';
  return b1 == 3 ? 'z' : b0 == 3 ? 'x' : 'h';
}

__global__ __launch_bounds__(256) void k_call_refspace(const CallRec *__restrict__ recs, int64_t nrec,
                                                       const uint32_t *__restrict__ cigar, const uint8_t *__restrict__ gseq,
                                                       const int64_t *__restrict__ goff, uint8_t *__restrict__ ref) {
  __shared__ CigarLds s_cig[kWaves];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kWaves + w;
  if (r >= nrec) return;                              // (whole waves: no workgroup barrier below)
  const CallRec c = recs[r];
  const int64_t g0 = goff[c.tid], glen = goff[c.tid + 1] - g0;
  const uint8_t *g = gseq + g0;
  uint8_t *out = ref + c.xm_off + 4 * r;              // out[2 + q]: query base q; out[0, 1] and out[l_seq + 2, 3]: halo
  auto base_at = [&](int64_t gi) -> uint8_t { return (uint8_t)((gi >= 0 && gi < glen ? g[gi] : 'N') & 7); };
  const uint32_t rlen = wave_cigar_walk(cigar + c.cig_off, c.n_cig, c.l_seq, s_cig[w], lane, [&](uint32_t q, uint32_t op, uint32_t rq) {
    out[2 + q] = (op == 0 || op == 7) ? base_at((int64_t)c.pos + rq) : (uint8_t)('N' & 7);
  });
  if (lane < 4) {
    const int64_t gi = lane < 2 ? (int64_t)c.pos - 2 + lane : (int64_t)c.pos + rlen + (lane - 2);
    out[lane < 2 ? lane : c.l_seq + lane] = base_at(gi);
  }
}

template <CallForm kForm>
__global__ __launch_bounds__(256) void k_call_xm(const CallRec *__restrict__ recs, int64_t nrec, const uint8_t *__restrict__ seq,
                                                 const uint8_t *__restrict__ ref, uint8_t *__restrict__ xm) {
  __shared__ uint8_t s_ctx[2][512];                  // [0]: forward table, [1]: reverse table
  for (int i = threadIdx.x; i < 512; i += 256) {
    s_ctx[0][i] = ctx_forward_dev((uint32_t)i >> 6, ((uint32_t)i >> 3) & 7, (uint32_t)i & 7);
    s_ctx[1][i] = ctx_reverse_dev((uint32_t)i >> 6, ((uint32_t)i >> 3) & 7, (uint32_t)i & 7);
  }
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * kWaves + w;
  if (r >= nrec) return;
  const CallRec c = recs[r];
  const uint8_t *rf = ref + c.xm_off + 4 * r;
  const uint8_t *sq = seq + c.seq_off;
  const int t = c.s_meth == 'C' ? 0 : 1;
  const int sh = t == 0 ? 2 : 0;                      // the triad starts at query base q (forward) or q - 2 (reverse)
  const uint8_t meth = c.s_meth, conv = c.s_conv;
  uint8_t *o = xm + c.xm_off;
  for (int32_t q = lane; q < c.l_seq; q += 64) {
    const uint32_t key = ((uint32_t)rf[q + sh] << 6) | ((uint32_t)rf[q + sh + 1] << 3) | (uint32_t)rf[q + sh + 2];
    uint8_t x = s_ctx[t][key];
    const uint8_t b = sq[q >> 1];
    const uint32_t nib = (q & 1) ? (b & 15u) : (b >> 4);
    if (x != '.') {
      // seq_nt16_str "=ACMGRSVTWYHKDBN": the base as a letter
      const uint8_t ch = (uint8_t)"=ACMGRSVTWYHKDBN"[nib];
      if (ch == meth) x &= 0xDF;
      else if (ch != conv) x = '.';
    }
    o[q] = kForm == CALL_PACKED ? (uint8_t)((nib << 4) | ctx_to_idx(x)) : x;
  }
}

}  // namespace


int call_methylation_window(epi_engine *eng, epi_genome *g, CallWork &wk, const CallRec *recs, int64_t nrec,
                            const uint32_t *cigar, int64_t ncig, const uint8_t *seq, int64_t nseq, int64_t nxm,
                            CallForm form, uint8_t *xm_out) {
  if (nrec <= 0) return EPI_OK;
  EPI_HIP(hipSetDevice(eng->device));
  const uint8_t *d_gseq = nullptr;
  const int64_t *d_goff = nullptr;
  EPI_TRY(genome_device(g, eng->device, &d_gseq, &d_goff));
  hipStream_t s = eng->stream;
  const int64_t nblk = (nrec + kWaves - 1) / kWaves;
  EPI_TRY(check_grid(nblk, 256, "callMethylation"));
  EPI_TRY(wk.recs.ensure((size_t)nrec * sizeof(CallRec)));
  EPI_TRY(wk.cig.ensure((size_t)(ncig > 0 ? ncig : 1) * sizeof(uint32_t)));
  EPI_TRY(wk.seq.ensure((size_t)(nseq > 0 ? nseq : 1)));
  EPI_TRY(wk.ref.ensure((size_t)nxm + 4 * (size_t)nrec));
  EPI_TRY(wk.xm.ensure((size_t)(nxm > 0 ? nxm : 1)));
  EPI_HIP(hipMemcpyAsync(wk.recs.p, recs, (size_t)nrec * sizeof(CallRec), hipMemcpyHostToDevice, s));
  if (ncig > 0) EPI_HIP(hipMemcpyAsync(wk.cig.p, cigar, (size_t)ncig * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  if (nseq > 0) EPI_HIP(hipMemcpyAsync(wk.seq.p, seq, (size_t)nseq, hipMemcpyHostToDevice, s));
  prof_begin("call_methylation", s);
  hipLaunchKernelGGL(k_call_refspace, dim3((unsigned)nblk), dim3(256), 0, s, wk.recs.as<CallRec>(), nrec, wk.cig.as<uint32_t>(),
                     d_gseq, d_goff, wk.ref.as<uint8_t>());
  EPI_HIP(hipGetLastError());
  if (form == CALL_PACKED)
    hipLaunchKernelGGL(k_call_xm<CALL_PACKED>, dim3((unsigned)nblk), dim3(256), 0, s, wk.recs.as<CallRec>(), nrec,
                       wk.seq.as<uint8_t>(), wk.ref.as<uint8_t>(), wk.xm.as<uint8_t>());
  else
    hipLaunchKernelGGL(k_call_xm<CALL_XM>, dim3((unsigned)nblk), dim3(256), 0, s, wk.recs.as<CallRec>(), nrec,
                       wk.seq.as<uint8_t>(), wk.ref.as<uint8_t>(), wk.xm.as<uint8_t>());
  EPI_HIP(hipGetLastError());
  prof_end("call_methylation", s);
  if (nxm > 0) EPI_TRY(copy_to_host(eng, xm_out, wk.xm.p, (size_t)nxm, s));
  EPI_HIP(hipStreamSynchronize(s));
  return EPI_OK;
}

}  // namespace epi
