// BLS12-381 scalar field Fr for gfx950 (CDNA4): the field of KZG blob polynomials
// (consensus-specs deneb polynomial-commitments.md BLS_MODULUS, the oracle's R).
//
// An element is 8 x 32-bit limbs (little-endian limb order) in Montgomery form,
// R = 2^256, always fully reduced to [0, r).  One lane owns one element, integer
// VALU only, in the style of bls_field.h; the 255-bit product is CIOS in plain
// C++ (64-bit accumulators, i.e. v_mad_u64_u32): 2 x 64 multiply-adds.  r < 2^255,
// so a sum of two elements fits the 8 limbs and the CIOS result is below 2r.
//
// fr_mul stays out of line with a register calling convention (8-wide vectors in,
// one out), for the reason bls_field.h gives for fp_mul: one body in the
// instruction cache, and no by-reference argument through scratch memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bls_constants.h"

#ifndef LB_DEV
#define LB_DEV __device__ __forceinline__
#define LB_NOINL __device__ __noinline__
#endif

namespace lb {

struct fr {
  uint32_t l[8];
};
typedef uint32_t fr_v __attribute__((ext_vector_type(8)));

static constexpr uint32_t FR_[8] = LB_FR_LIMBS;

LB_DEV void fr_set(fr& r, const uint32_t* c) {
#pragma unroll
  for (int j = 0; j < 8; j++) r.l[j] = c[j];
}
LB_DEV void fr_zero(fr& r) {
#pragma unroll
  for (int j = 0; j < 8; j++) r.l[j] = 0;
}
LB_DEV void fr_one(fr& r) { fr_set(r, LB_FR_ONE); }
LB_DEV bool fr_is_zero(const fr& a) {
  uint32_t acc = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) acc |= a.l[j];
  return acc == 0;
}
LB_DEV bool fr_eq(const fr& a, const fr& b) {
  uint32_t acc = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) acc |= a.l[j] ^ b.l[j];
  return acc == 0;
}

// t - r into s; returns the borrow (1: t < r)
LB_DEV uint32_t fr_sub_r(uint32_t* s, const uint32_t* t) {
  uint32_t br = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint64_t d = (uint64_t)t[j] - FR_[j] - br;
    s[j] = (uint32_t)d;
    br = (uint32_t)(d >> 63);
  }
  return br;
}
// r = t - r if t >= r else t   (t < 2r, t < 2^256)
LB_DEV void fr_csub(fr& r, const uint32_t* t) {
  uint32_t s[8];
  const uint32_t br = fr_sub_r(s, t);
#pragma unroll
  for (int j = 0; j < 8; j++) r.l[j] = br ? t[j] : s[j];
}

LB_DEV void fr_add(fr& r, const fr& a, const fr& b) {
  uint32_t t[8];
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint64_t s = (uint64_t)a.l[j] + b.l[j] + c;
    t[j] = (uint32_t)s;
    c = (uint32_t)(s >> 32);
  }
  fr_csub(r, t);  // (a + b < 2r < 2^256: no carry out of limb 7)
}
LB_DEV void fr_sub(fr& r, const fr& a, const fr& b) {
  uint32_t t[8];
  uint32_t br = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint64_t d = (uint64_t)a.l[j] - b.l[j] - br;
    t[j] = (uint32_t)d;
    br = (uint32_t)(d >> 63);
  }
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint64_t s = (uint64_t)t[j] + (br ? FR_[j] : 0u) + c;
    r.l[j] = (uint32_t)s;
    c = (uint32_t)(s >> 32);
  }
}
LB_DEV void fr_neg(fr& r, const fr& a) {
  fr z;
  fr_zero(z);
  fr_sub(r, z, a);
}

// Montgomery product a b R^-1 mod r (CIOS), fully reduced; a, b < r
LB_NOINL fr_v fr_mul_r(fr_v a, fr_v b) {
  uint32_t t[10];
#pragma unroll
  for (int j = 0; j < 10; j++) t[j] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint64_t s = (uint64_t)a[j] * b[i] + t[j] + c;
      t[j] = (uint32_t)s;
      c = s >> 32;
    }
    uint64_t s = (uint64_t)t[8] + c;
    t[8] = (uint32_t)s;
    t[9] = (uint32_t)(s >> 32);
    const uint32_t m = t[0] * LB_FR_INV32;
    c = ((uint64_t)m * FR_[0] + t[0]) >> 32;
#pragma unroll
    for (int j = 1; j < 8; j++) {
      s = (uint64_t)m * FR_[j] + t[j] + c;
      t[j - 1] = (uint32_t)s;
      c = s >> 32;
    }
    s = (uint64_t)t[8] + c;
    t[7] = (uint32_t)s;
    t[8] = t[9] + (uint32_t)(s >> 32);
  }
  // t < 2r < 2^256 (t[8] == 0)
  fr o;
  fr_csub(o, t);
  fr_v v;
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] = o.l[j];
  return v;
}
LB_DEV fr_v fr_pack(const fr& a) {
  fr_v v;
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] = a.l[j];
  return v;
}
LB_DEV void fr_mul(fr& r, const fr& a, const fr& b) {
  const fr_v v = fr_mul_r(fr_pack(a), fr_pack(b));
#pragma unroll
  for (int j = 0; j < 8; j++) r.l[j] = v[j];
}
LB_DEV void fr_sqr(fr& r, const fr& a) { fr_mul(r, a, a); }
LB_DEV void fr_mul_const(fr& r, const fr& a, const uint32_t* c) {
  fr k;
  fr_set(k, c);
  fr_mul(r, a, k);
}
// raw (< r) -> Montgomery, and back
LB_DEV void fr_to_mont(fr& r, const fr& a) { fr_mul_const(r, a, LB_FR_R2); }
LB_DEV void fr_from_mont(fr& r, const fr& a) {
  fr one_raw;
  fr_zero(one_raw);
  one_raw.l[0] = 1;
  fr_mul(r, a, one_raw);
}

// a^e for a 256-bit exponent (8 limbs, little-endian), left to right
LB_DEV void fr_pow(fr& r, const fr& a, const uint32_t* e) {
  fr acc;
  fr_one(acc);
  const fr base = a;
#pragma unroll 1
  for (int i = 255; i >= 0; i--) {
    fr_sqr(acc, acc);
    if ((e[i >> 5] >> (i & 31)) & 1u) fr_mul(acc, acc, base);
  }
  r = acc;
}
// a^(r-2): 1/a, and 0 for a = 0
LB_DEV void fr_inv(fr& r, const fr& a) {
  uint32_t e[8];
  uint32_t br = 2;  // (r's low limb is 1: the subtraction borrows into limb 1)
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint64_t d = (uint64_t)FR_[j] - br;
    e[j] = (uint32_t)d;
    br = (uint32_t)(d >> 63);
  }
  fr_pow(r, a, e);
}

// ---- byte codecs (32 bytes, big-endian) -----------------------------------
LB_DEV void fr_raw_from_be32(uint32_t* t, const uint8_t* b) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint8_t* p = b + 4 * (7 - j);
    t[j] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
  }
}
// raw limbs (little-endian) < r ?
LB_DEV bool fr_raw_is_canonical(const uint32_t* t) {
  uint32_t s[8];
  return fr_sub_r(s, t) != 0;
}
// bytes_to_bls_field: false (and r = 0) for a value >= r
LB_DEV bool fr_from_be32(fr& r, const uint8_t* b) {
  uint32_t t[8];
  fr_raw_from_be32(t, b);
  const bool ok = fr_raw_is_canonical(t);
  fr raw;
#pragma unroll
  for (int j = 0; j < 8; j++) raw.l[j] = ok ? t[j] : 0u;
  fr_to_mont(r, raw);
  return ok;
}
// hash_to_bls_field: any 256-bit value (8 big-endian words, as SHA-256 leaves its digest)
// reduced mod r; 2^256 < 3r, so two conditional subtractions
LB_DEV void fr_from_be_words_reduce(fr& r, const uint32_t* w) {
  uint32_t t[8], s[8];
#pragma unroll
  for (int j = 0; j < 8; j++) t[j] = w[7 - j];
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const uint32_t br = fr_sub_r(s, t);
#pragma unroll
    for (int j = 0; j < 8; j++) t[j] = br ? t[j] : s[j];
  }
  fr raw;
#pragma unroll
  for (int j = 0; j < 8; j++) raw.l[j] = t[j];
  fr_to_mont(r, raw);
}
// canonical big-endian bytes
LB_DEV void fr_to_be32(uint8_t* out, const fr& a) {
  fr raw;
  fr_from_mont(raw, a);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint32_t v = raw.l[7 - j];
    out[4 * j] = (uint8_t)(v >> 24);
    out[4 * j + 1] = (uint8_t)(v >> 16);
    out[4 * j + 2] = (uint8_t)(v >> 8);
    out[4 * j + 3] = (uint8_t)v;
  }
}

}  // namespace lb
