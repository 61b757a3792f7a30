// csrc/xm_codes.hpp on the host: the two table lookups over a model of v_perm_b32's selector rules (selector 0-7: a byte of
// {S0, S1}; 8-11: the sign of byte 1 / 3 / 5 / 7 spread over the byte; 12: 0x00; >= 13: 0xFF -- the rules lut16_xor_form's
// comment states), the code of every XM letter, the two class masks and the read rule's verdict on its seams.  Built with
// -fsanitize=address,undefined and run as a program of its own (tests/test_xm_codes.py).
#include <stdint.h>
#include <stdio.h>
#include <cmath>
#include <random>

static uint32_t perm_model(uint32_t s0, uint32_t s1, uint32_t sel) {
  uint8_t in[8];
  for (int i = 0; i < 4; i++) { in[i] = (uint8_t)(s1 >> (8 * i)); in[4 + i] = (uint8_t)(s0 >> (8 * i)); }
  uint32_t r = 0;
  for (int i = 0; i < 4; i++) {
    const uint8_t s = (uint8_t)(sel >> (8 * i));
    const uint8_t b = s >= 13 ? 0xFF : s == 12 ? 0x00 : s >= 8 ? ((in[2 * (s - 8) + 1] & 0x80) ? 0xFF : 0x00) : in[s];
    r |= (uint32_t)b << (8 * i);
  }
  return r;
}
#define XM_CODES_HOST_PERM perm_model
#include "xm_codes.hpp"

using namespace epi;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

int main() {
  // the lookups: every code in every byte lane of a few hundred random tables
  std::mt19937 rng(20240611);
  for (int it = 0; it < 300; it++) {
    uint8_t f[16];
    for (int c = 0; c < 16; c++) f[c] = (uint8_t)(rng() & (it % 3 == 0 ? 0x7Fu : 0xFFu));   // (the kernels' tables: entries below 128)
    const ClassLut d = lut16_pack(f), x = lut16_xor_form(d);
    for (int lane = 0; lane < 4; lane++)
      for (uint32_t c = 0; c < 16; c++) {
        const uint32_t noise = rng();                          // the other lanes' codes and every high nibble: anything
        const uint32_t w = (noise & ~(0xFu << (8 * lane))) | (c << (8 * lane));
        const auto byte = [&](uint32_t v) { return (v >> (8 * lane)) & 255u; };
        CHECK(byte(lut16_pick(w, d)) == f[c], "pick: table %d lane %d code %u", it, lane, c);
        CHECK(byte(lut16_pick(w, d, 0x07060504u)) == f[c | 8u], "pick, upper half: table %d lane %d code %u", it, lane, c);
        CHECK(byte(lut16_xor(w, x)) == f[c], "xor: table %d lane %d code %u", it, lane, c);
        CHECK(byte(lut16_xor(w, x, 0x08080808u)) == f[c | 8u], "xor, low8: table %d lane %d code %u", it, lane, c);
        CHECK(plane_nibble(w, 3) == plane_nibble_mul(w, 3), "nibble gathers: %08x", w);
      }
  }

  // the letters
  const struct { char c; unsigned code; } letters[] = {{'z', 15}, {'Z', 7}, {'x', 14}, {'X', 6}, {'h', 10}, {'H', 2}, {'u', 13}, {'U', 5},
                                                       {'.', kXmDot}, {'+', kXmSkip}, {'-', kXmSkip}};
  for (const auto &l : letters) CHECK(ctx_to_idx((unsigned char)l.c) == l.code, "ctx_to_idx('%c') = %u", l.c, ctx_to_idx((unsigned char)l.c));
  CHECK(ctx_mask_of("Zz") == ((1u << 7) | (1u << 15)), "ctx_mask_of(Zz)");
  CHECK(kXmDot4 == 0x01010101u * kXmDot, "filler");

  // the classes
  uint32_t meth = 0, unmeth = 0;
  for (unsigned c : {2u, 5u, 6u, 7u}) meth |= 1u << c;
  for (unsigned c : {10u, 13u, 14u, 15u}) unmeth |= 1u << c;
  CHECK(kXmMethMask == meth && kXmUnmethMask == unmeth, "class masks %04x %04x", kXmMethMask, kXmUnmethMask);
  uint32_t oom = 0, oou = 0;
  ooctx_masks(ctx_mask_of("Zz"), &oom, &oou);
  CHECK(oom == (meth & ~(1u << 7)) && oou == (unmeth & ~(1u << 15)), "ooctx_masks %04x %04x", oom, oou);

  // the verdict
  CHECK(read_rule_keeps(10, 0, 0, 0.1), "0 / 0 is NaN: kept");
  CHECK(read_rule_keeps(10, 0, 0, std::nan("")) && read_rule_keeps(10, 3, 1, std::nan("")), "a NaN threshold drops nothing");
  CHECK(!read_rule_keeps(0, 0, 0, 0.1) && !read_rule_keeps(0, 0, 5, 1.0) && !read_rule_keeps(-1, 0, 5, 1.0), "an empty row is dropped");
  CHECK(read_rule_keeps(10, 1, 3, 0.25), "frac == max_oo: kept");
  CHECK(!read_rule_keeps(10, 1, 3, std::nextafter(0.25, 0.0)), "frac just above max_oo: dropped");
  CHECK(read_rule_keeps(10, 1, 9, 0.1) == !(1.0 / 10.0 > 0.1), "1 / 10 against 0.1: one IEEE division, compared as is");
  CHECK(read_rule_keeps(1, 5, 0, 1.0) && !read_rule_keeps(1, 5, 0, std::nextafter(1.0, 0.0)), "all methylated");
  // om + ou near 2^32: the sum is taken in 64 bits
  CHECK(!read_rule_keeps(1, 0xFFFFFFFFu, 0xFFFFFFFFu, 0.25), "2^32 - 1 of each: 0.5, not a wrapped sum");
  CHECK(read_rule_keeps(1, 0xFFFFFFFFu, 0xFFFFFFFFu, 0.5), "2^32 - 1 of each: exactly 0.5");
  CHECK(read_rule_keeps(1, 1, 0xFFFFFFFFu, 1.0 / 4294967296.0) && !read_rule_keeps(1, 2, 0xFFFFFFFEu, 1.0 / 4294967296.0),
        "1 and 2 of 2^32 against 2^-32");

  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("xm_codes ok\n");
  return 0;
}
