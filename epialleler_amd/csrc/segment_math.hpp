// The arithmetic of the methylation-segment HMM (include/epihip.h, epi_cx_segment_dev, has the model): host and device, plain
// C++, templated on the number of states K.  Everything is an integer: log-probabilities are fixed point (2^-16 units), max and
// + on integers are exactly associative, so a blocked scan over these pieces gives the path and the score of the plain loop at
// every tie.  segment_host.cpp (the loop) and segment.hip (the scans) both include this; nothing else restates it.
//  Tables    A[k] = q(p[k]), B[k] = q(1 - p[k]), T[j][k] = q(trans[j][k]), I[k] = q(init[k]), all <= 0.
//  Bound     a call takes at most 2^26 sites and counts of at most 32767 per site.  A and B are >= q(2^-16) = -726817 (p is
//            clamped at every refit); T and I are >= -2^21 (-726817 for a caller's parameters; a refitted transition or
//            start is >= q(1 / (2^26 + 4)) = -1181078).  A site then adds at least -(32767 * 726817 + 2^21) > -2^35 to a
//            score, so every partial score lies in (-2^62, 0] and no sum here can overflow.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SEG_HD __host__ __device__ __forceinline__
#else
#define SEG_HD inline
#endif
#if defined(__clang__)
#define SEG_UNROLL _Pragma("unroll")
#else
#define SEG_UNROLL
#endif

namespace epi {
namespace segment {

constexpr int kMaxStates = 4;
constexpr int32_t kMinEmission = -726817;                      // q(2^-16): the least entry of A and B
constexpr int32_t kMinTable = -(1 << 21);                      // the least entry of T and I

// the tables of one model as the kernels take them (by value); unused entries are 0
struct Tables { int32_t A[kMaxStates], B[kMaxStates], T[kMaxStates * kMaxStates], I[kMaxStates]; };

constexpr int table_words(int K) { return 3 * K + K * K; }     // A, B, T (row-major), I back to back
constexpr int count_words(int K) { return 3 * K + K * K; }     // M, U, N (row-major), S back to back

template <int K> SEG_HD void tables_unpack(const int32_t *w, Tables &t) {
SEG_UNROLL
  for (int k = 0; k < K; k++) { t.A[k] = w[k]; t.B[k] = w[K + k]; t.I[k] = w[2 * K + K * K + k]; }
SEG_UNROLL
  for (int x = 0; x < K * K; x++) t.T[(x / K) * kMaxStates + x % K] = w[2 * K + x];
}

// The coverage clip: the counts the model sees.  Both fit 15 bits.
SEG_HD void clip_counts(int32_t meth, int32_t unmeth, int32_t max_coverage, int32_t *m, int32_t *u) {
  const int64_t cov = (int64_t)meth + (int64_t)unmeth;
  if (cov > (int64_t)max_coverage) {
    const int32_t mc = (int32_t)(((int64_t)meth * (int64_t)max_coverage) / cov);
    *m = mc; *u = max_coverage - mc;
  } else {
    *m = meth; *u = unmeth;
  }
}

// a site as one word: m' in bits 0 .. 14, u' in bits 16 .. 30, bit 31 set at the first site of a chain
SEG_HD uint32_t site_pack(int32_t m, int32_t u, bool head) { return (uint32_t)m | ((uint32_t)u << 16) | (head ? 0x80000000u : 0u); }
SEG_HD int32_t site_m(uint32_t w) { return (int32_t)(w & 0x7FFFu); }
SEG_HD int32_t site_u(uint32_t w) { return (int32_t)((w >> 16) & 0x7FFFu); }
SEG_HD bool site_head(uint32_t w) { return (w >> 31) != 0; }

template <int K> struct Vec { int64_t v[K]; };
template <int K> struct Mat { int64_t a[K * K]; };             // a[j * K + k]: from state j to state k

// e(k) = m' A[k] + u' B[k]
template <int K> SEG_HD void emission(const Tables &t, int32_t m, int32_t u, Vec<K> &e) {
SEG_UNROLL
  for (int k = 0; k < K; k++) e.v[k] = (int64_t)m * (int64_t)t.A[k] + (int64_t)u * (int64_t)t.B[k];
}

// delta_0(k) = I[k] + e(k)
template <int K> SEG_HD void first_step(const Tables &t, const Vec<K> &e, Vec<K> &d) {
SEG_UNROLL
  for (int k = 0; k < K; k++) d.v[k] = (int64_t)t.I[k] + e.v[k];
}

// One Viterbi step: d(k) <- max_j (d(j) + T[j][k]) + e(k); returns the psi byte, 2 bits per state k: the SMALLEST j that
// attains the maximum.
template <int K> SEG_HD uint32_t viterbi_step(const Tables &t, const Vec<K> &e, Vec<K> &d) {
  Vec<K> nd;
  uint32_t psi = 0;
SEG_UNROLL
  for (int k = 0; k < K; k++) {
    int64_t best = d.v[0] + (int64_t)t.T[k];
    uint32_t arg = 0;
SEG_UNROLL
    for (int j = 1; j < K; j++) {
      const int64_t x = d.v[j] + (int64_t)t.T[j * kMaxStates + k];
      if (x > best) { best = x; arg = (uint32_t)j; }
    }
    nd.v[k] = best + e.v[k];
    psi |= arg << (2 * k);
  }
  d = nd;
  return psi;
}

// the largest entry and the SMALLEST state that attains it
template <int K> SEG_HD uint32_t best_state(const Vec<K> &d, int64_t *score) {
  int64_t best = d.v[0];
  uint32_t arg = 0;
SEG_UNROLL
  for (int k = 1; k < K; k++) if (d.v[k] > best) { best = d.v[k]; arg = (uint32_t)k; }
  *score = best;
  return arg;
}

// The max-plus matrix of a site inside a chain, M[j][k] = T[j][k] + e(k), and of a chain's first site, H[j][k] = I[k] + e(k)
// for every j (whatever came before is forgotten).
template <int K> SEG_HD void site_matrix(const Tables &t, const Vec<K> &e, bool head, Mat<K> &m) {
SEG_UNROLL
  for (int j = 0; j < K; j++)
SEG_UNROLL
    for (int k = 0; k < K; k++) m.a[j * K + k] = (head ? (int64_t)t.I[k] : (int64_t)t.T[j * kMaxStates + k]) + e.v[k];
}

// the max-plus product, first x then y: (x * y)[j][k] = max_l (x[j][l] + y[l][k])
template <int K> SEG_HD void maxplus(const Mat<K> &x, const Mat<K> &y, Mat<K> &out) {
  Mat<K> r;
SEG_UNROLL
  for (int j = 0; j < K; j++)
SEG_UNROLL
    for (int k = 0; k < K; k++) {
      int64_t best = x.a[j * K] + y.a[k];
SEG_UNROLL
      for (int l = 1; l < K; l++) {
        const int64_t v = x.a[j * K + l] + y.a[l * K + k];
        best = v > best ? v : best;
      }
      r.a[j * K + k] = best;
    }
  out = r;
}

// a vector through a matrix: (d * y)[k] = max_l (d[l] + y[l][k])
template <int K> SEG_HD void maxplus_vec(const Vec<K> &d, const Mat<K> &y, Vec<K> &out) {
  Vec<K> r;
SEG_UNROLL
  for (int k = 0; k < K; k++) {
    int64_t best = d.v[0] + y.a[k];
SEG_UNROLL
    for (int l = 1; l < K; l++) {
      const int64_t v = d.v[l] + y.a[l * K + k];
      best = v > best ? v : best;
    }
    r.v[k] = best;
  }
  out = r;
}

// Maps of states as bytes, 2 bits per argument: map(k) = (byte >> 2k) & 3.  A psi byte is the map from a site's state to its
// predecessor's.
constexpr uint32_t kIdentityMap = 0xE4u;
SEG_HD uint32_t map_apply(uint32_t map, uint32_t k) { return (map >> (2 * k)) & 3u; }
SEG_HD uint32_t map_constant(uint32_t state) { return state * 0x55u; }
// f after g: (f o g)(k) = f(g(k))
SEG_HD uint32_t map_compose(uint32_t f, uint32_t g) {
  uint32_t r = 0;
SEG_UNROLL
  for (int k = 0; k < kMaxStates; k++) r |= map_apply(f, map_apply(g, (uint32_t)k)) << (2 * k);
  return r;
}

// segment_host.cpp, built without fast-math and without contraction: q(x) = floor(log(x) * 65536 + 0.5) over a model's
// parameters with no range check (a refitted transition may lie below 2^-16), table_words(K) words out; and the hard-EM
// re-estimate of epi_segment_reestimate.
int check_model(const char *who, int32_t K, const double *p, const double *trans, const double *init);   // a caller's model: EPI_ERR_ARG or EPI_OK
void quantise_tables(int K, const double *p, const double *trans, const double *init, int32_t *tables_out);
void reestimate(int K, const int64_t *counts, double *p, double *trans, double *init);

}  // namespace segment
}  // namespace epi
