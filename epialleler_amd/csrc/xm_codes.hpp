// The packed XM code alphabet: what the 16 nibble codes mean, the 16-entry byte table over them (ClassLut) with its two
// v_perm_b32 lookups, and the lMHL read rule's verdict.  Plain host C++ (common.hpp includes it); the lookups are device functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace epi {

// ---- the codes ---------------------------------------------------------------------------------------------------------
// A packed byte's low nibble is ctx_to_idx of the XM letter: H X Z = 2 6 7, h x z = 10 14 15 (code & 7: the context, code < 8:
// methylated), U u = 5 13, '+' '-' = 11, '.' = 12.
__host__ __device__ inline unsigned ctx_to_idx(unsigned char c) { return ((unsigned(c) + 2u) >> 2) & 15u; }   // src/epialleleR.h:28
// the codes of a report's context string as a bit mask (rcpp_cx_report.cpp:88-91, rcpp_mhl_report.cpp:104-107)
inline uint32_t ctx_mask_of(const char *ctx) {
  uint32_t ctx_mask = 0;
  for (const unsigned char *c = reinterpret_cast<const unsigned char *>(ctx); *c; c++) ctx_mask |= 1u << ctx_to_idx(*c);
  return ctx_mask;
}
constexpr uint32_t kXmMethMask = 0x00E4u;      // the methylated codes 2, 5, 6, 7 as a bit mask (rcpp_mhl_report.cpp:176)
constexpr uint32_t kXmUnmethMask = 0xE400u;    // the unmethylated codes 10, 13, 14, 15 (:177)
constexpr uint32_t kXmSkip = 11;               // '+' / '-' and the filler between mates: skipped (rcpp_cx_report.cpp:123, rcpp_mhl_report.cpp:187)
constexpr uint32_t kXmDot = 12;                // '.': in no class, never a call
constexpr uint32_t kXmDot4 = 0x0C0C0C0Cu;      // ... in every byte of a dword: what a byte outside the row reads as

// the read rule's out-of-context methylated / unmethylated codes: those of either class that are not in the context
inline void ooctx_masks(uint32_t ctx_mask, uint32_t *oom, uint32_t *oou) {
  *oom = kXmMethMask & ~ctx_mask;              // rcpp_mhl_report.cpp:176-177
  *oou = kXmUnmethMask & ~ctx_mask;
}

// The verdict of the lMHL read rule, hmin = 0 (rcpp_mhl_report.cpp:172-179), on a row of len bytes with om / ou out-of-context
// methylated / unmethylated bytes: 0 / 0 is NaN and keeps the row.  (max_oo by reference: kernels read it where it is compared.)
__host__ __device__ inline bool read_rule_keeps(int32_t len, uint32_t om, uint32_t ou, const double &max_oo) {
  const double frac = (double)om / (double)((uint64_t)om + ou);
  return len > 0 && !(frac > max_oo);
}

// ---- the 16-entry byte table ---------------------------------------------------------------------------------------------
struct ClassLut { uint32_t lo0, lo1, hi0, hi1; };   // one byte per code: codes 0-3, 4-7, 8-11, 12-15
template <class T> inline ClassLut lut16_pack(const T (&f)[16]) {   // f[code]: the code's byte (its low eight bits)
  uint32_t w[4] = {0, 0, 0, 0};
  for (int c = 0; c < 16; c++) w[c >> 2] |= ((uint32_t)f[c] & 255u) << (8 * (c & 3));
  return ClassLut{w[0], w[1], w[2], w[3]};
}

// The same table in the form two v_perm_b32 look up (lut16_xor).  With a selector byte s, v_perm_b32 returns
// byte s of its eight source bytes for s < 8, the sign of source byte 1 / 3 / 5 / 7 spread over the byte for s = 8 .. 11,
// 0x00 for s = 12 and 0xFF for s >= 13.  So perm(low half, code) is the entry for codes 0 .. 7 and a constant per code
// for 8 .. 15, perm(high half, code ^ 8) the other way round; the halves are stored XOR-ed with the constant the other
// lookup returns, and the XOR of the two lookups is the entry for every code.
inline ClassLut lut16_xor_form(const ClassLut &d) {
  uint8_t D[16], X[16], *L = X, *H = X + 8;
  const uint32_t w[4] = {d.lo0, d.lo1, d.hi0, d.hi1};
  for (int c = 0; c < 16; c++) D[c] = (uint8_t)(w[c >> 2] >> (8 * (c & 3)));
  auto S = [](uint8_t x) { return (uint8_t)((x & 0x80u) ? 0xFFu : 0x00u); };
  L[4] = D[4]; H[4] = D[12];
  for (int j = 5; j < 8; j++) { L[j] = (uint8_t)~D[j]; H[j] = (uint8_t)~D[8 + j]; }
  L[2] = D[2] ^ S(H[5]); L[3] = D[3] ^ S(H[7]); H[2] = D[10] ^ S(L[5]); H[3] = D[11] ^ S(L[7]);
  L[1] = D[1] ^ S(H[3]); H[1] = D[9] ^ S(L[3]);
  L[0] = D[0] ^ S(H[1]); H[0] = D[8] ^ S(L[1]);
  return lut16_pack(X);
}

// ---- the lookups: the table's bytes of the four codes (low nibbles) of a dword --------------------------------------------
// Device functions over the instruction's builtin (called directly: a wrapper function around it changes a kernel's code).  A host
// program that defines XM_CODES_HOST_PERM as its model of the instruction gets the same expressions (tests/cpp/xm_codes_main.cpp).
#if defined(__HIPCC__)
#define XM_CODES_FN __device__ __forceinline__
#define XM_V_PERM __builtin_amdgcn_perm
#elif defined(XM_CODES_HOST_PERM)
#define XM_CODES_FN inline
#define XM_V_PERM XM_CODES_HOST_PERM
#endif
#ifdef XM_CODES_FN

// Three v_perm_b32: codes 0-7 and 8-15 are looked up by their low three bits, and a third perm picks, per byte, the second
// result when bit 3 of the code is set (selector j + 4 * bit3): no multiply, no masks.  pick0 = 0x07060504 takes the
// codes-8..15 result for every byte (a lower-cased read, code | 8).
XM_CODES_FN uint32_t lut16_pick(uint32_t w, const ClassLut &F, uint32_t pick0 = 0x03020100u) {
  const uint32_t lo3 = w & 0x07070707u;
  const uint32_t pick = ((w >> 1) & 0x04040404u) | pick0;
  return XM_V_PERM(XM_V_PERM(F.hi1, F.hi0, lo3), XM_V_PERM(F.lo1, F.lo0, lo3), pick);
}

// Two v_perm_b32 over a table in lut16_xor_form; low8 = 0 or, for a lower-cased read, 0x08080808 (every byte takes the entry
// of code | 8, rcpp_cx_report.cpp:118,122)
XM_CODES_FN uint32_t lut16_xor(uint32_t w, const ClassLut &X, uint32_t low8 = 0u) {
  const uint32_t sel = (w & 0x0F0F0F0Fu) | low8;
  return XM_V_PERM(X.lo1, X.lo0, sel) ^ XM_V_PERM(X.hi1, X.hi0, sel ^ 0x08080808u);
}

// Bit `bit` of the four bytes of f as a nibble (byte j -> bit j), twice: the instruction sequences differ and each stays with
// the kernels measured with it.  plane_nibble, shifts and ORs, is the lMHL kernels' (mhl_report.hip, mhl_fused.hip);
// plane_nibble_mul, one multiply whose products' bits do not meet, is the allele-specific report's walk (asm_report.hip).
XM_CODES_FN uint32_t plane_nibble(uint32_t f, int bit) {
  uint32_t t = (f >> bit) & 0x01010101u;
  t |= t >> 7;
  t |= t >> 14;
  return t & 0xFu;
}
XM_CODES_FN uint32_t plane_nibble_mul(uint32_t f, int bit) { return (((f >> bit) & 0x01010101u) * 0x01020408u) >> 24; }

#endif  // XM_CODES_FN

}  // namespace epi
