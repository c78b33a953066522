// a^((p-3)/4) on carry-free 30-bit columns (DESIGN.md §4 "Field core").
//
// The one exponentiation behind fp_sqrt, fp_is_square, fp2_sqrt and the hash's square-root
// fractions is 486 dependent field operations on one element, 378 of them squarings.  Inside it
// the element lives as 13 digits of 30 bits: a digit product is < 2^60, so a whole column of up
// to 13 products (13 x 2^60 < 2^64) accumulates in one 64-bit register with v_mad_u64_u32 alone,
// where the 12 x 32-bit product scanning of bls_fp_ps.h pays a v_addc_co_u32 behind every mad.
// One element enters the layout, stays for the whole chain and leaves: no digit conversion, no
// conditional subtraction and no call marshalling per operation.  A resident squaring is
// 91 + 169 mads, a resident product 169 + 169.
//
// Radix.  Inside the chain the Montgomery radix is 2^390 = 2^(13 x 30): the reduction takes 13
// whole digits and the result needs no realignment.  Callers use R = 2^384, and see exactly
// what the limb code returns, a^((p-3)/4) R mod p, canonical (< p):
//   entry  the caller's x = a R is read as it stands, as the 2^390-form of a' = a 2^-6;
//   chain  gives a'^e 2^390 = a^e 2^(-6e) 2^390, with e = (p-3)/4;
//   exit   one more resident product by the constant LB_POW_EXIT30 = 2^(384 + 6e) mod p
//          (gen_constants.py) gives a^e 2^384; then digits -> limbs and one subtraction of p.
//
// Bounds.  A resident operation returns (x y + m p) / 2^390 with m < 2^390, so for operands
// < 2p the result is < 4p^2 / 2^390 + p < 1.01 p (p < 2^381): operands < 2p give a result
// < 2p with no conditional subtraction anywhere in the chain.  The first step holds too: the
// entry value is a 12-limb word, so < 2^384, and 2^768 / 2^390 + p < 2p.  Digits are always
// normalised (< 2^30); only the exit makes the value canonical.
// Column sums: the operands' digit products and the reduction's m_i p_j of a column (up to 13
// terms of < 2^60 each) do not fit one 64-bit word together, so each kind has its own chain and
// its own carry into the next column (mont() below).
//
// Measured on MI355X at two waves per SIMD (tools/microbench/fp_cols_bench.hip): squaring 2,091
// against 3,030 cycles per wave-operation, product 2,350 against 2,920, the whole exponentiation
// 1.20 M against 1.48 M.
//
// LB_HD: __device__ __forceinline__ in the library; plain inline C++ for the host tests
// (tests/native/pow_cols_host.cpp, tests/test_fp_pow_cols.py).
#pragma once
#include <stdint.h>

#ifndef LB_HD
#define LB_HD __device__ __forceinline__
#endif
// the counting build (bls_field.h, tools/opcount.py) prices one squaring or one product per
// resident operation, as it does for the limb code
#ifndef LB_COUNT_MUL
#define LB_COUNT_MUL() ((void)0)
#define LB_COUNT_SQR() ((void)0)
#endif

namespace lb {
namespace pw {

constexpr uint32_t M30 = (1u << 30) - 1;

struct d13 {
  uint32_t d[13];
};
// p (LB_P_LIMBS) as 13 digits of 30 bits
constexpr d13 p_digits() {
  constexpr uint32_t P32[12] = LB_P_LIMBS;
  d13 r{};
  for (int i = 0; i < 13; i++) {
    const int o = 30 * i, w = o / 32, s = o % 32;
    const uint64_t v = (uint64_t)(w < 12 ? P32[w] : 0u) | ((uint64_t)(w + 1 < 12 ? P32[w + 1] : 0u) << 32);
    r.d[i] = (uint32_t)(v >> s) & M30;
  }
  return r;
}
// -p^-1 mod 2^30 (Newton: each step doubles the correct low bits)
constexpr uint32_t p_inv30() {
  constexpr d13 P = p_digits();
  uint32_t inv = 1;
  for (int k = 0; k < 6; k++) inv *= 2u - P.d[0] * inv;
  return (0u - inv) & M30;
}
constexpr d13 PD = p_digits();
constexpr uint32_t PINV30 = p_inv30();
static_assert(((PD.d[0] * PINV30) & M30) == M30, "-p^-1 mod 2^30");
constexpr d13 EXIT = {LB_POW_EXIT30};

// 12 limbs -> 13 digits (any 12-limb value; digit 12 is bits 360 .. 383)
LB_HD void enter(d13& r, const uint32_t* a) {
#pragma unroll
  for (int i = 0; i < 13; i++) {
    const int o = 30 * i, w = o / 32, s = o % 32;
    const uint32_t lo = a[w] >> s;
    const uint32_t hi = (s > 2 && w + 1 < 12) ? a[w + 1] << (32 - s) : 0u;
    r.d[i] = (lo | hi) & M30;
  }
}
// 13 digits of a value < 2p -> 12 limbs, canonical (< p)
LB_HD void leave(uint32_t* r, const d13& a) {
  constexpr uint32_t P32[12] = LB_P_LIMBS;
  uint32_t t[12], s[12];
#pragma unroll
  for (int j = 0; j < 12; j++) {
    const int o = 32 * j, k = o / 30, sh = o % 30;
    uint32_t v = a.d[k] >> sh;
    v |= a.d[k + 1] << (30 - sh);  // sh = 2 j <= 22: two digits cover the limb; k + 1 <= 12
    t[j] = v;
  }
  uint32_t br = 0;
#pragma unroll
  for (int j = 0; j < 12; j++) {
    const uint64_t d = (uint64_t)t[j] - P32[j] - br;
    s[j] = (uint32_t)d;
    br = (uint32_t)(d >> 63);
  }
#pragma unroll
  for (int j = 0; j < 12; j++) r[j] = br ? t[j] : s[j];
}

// r = a b 2^-390 mod p, or a^2 2^-390 mod p (SQR; b unused): operands < 2p with digits < 2^30,
// r < 2p, and r may be a or b (digit k - 13 is written when neither operand's is read again).
// Product scanning, one column of weight 2^(30 k) at a time, on two 64-bit chains: ap takes the
// digit products of the operands, ar the m_i p_j of the reduction, each starting from its own
// carry out of the column below (the first mad's addend, so the carry costs no addition).
// Neither chain depends on the other except through m_k, so the products run ahead of the
// reduction.  The squaring takes the cross products once with a doubled factor (2 a_i < 2^31).
// Bounds: a column holds at most 13 products of < 2^60 (the squaring's 6 doubled ones and one
// square come to the same 13 x 2^60) and a carry < 2^34; ar also takes ap's low 30 bits:
// 13 x 2^60 + 2^34 + 2^30 < 2^64.
template <bool SQR>
LB_HD void mont(d13& r, const d13& a, const d13& b) {
  uint32_t a2[13], m[13];
  if (SQR) {
#pragma unroll
    for (int i = 0; i < 13; i++) a2[i] = a.d[i] << 1;
  }
  uint64_t cp = 0, cr = 0;
#pragma unroll
  for (int k = 0; k < 26; k++) {
    const int i0 = k < 13 ? 0 : k - 12, i1 = k < 13 ? k : 12;
    uint64_t ap = cp, ar = cr;
    if (SQR) {
#pragma unroll
      for (int i = i0; 2 * i < k; i++) ap += (uint64_t)a2[i] * a.d[k - i];
      if (k % 2 == 0 && k <= 24) ap += (uint64_t)a.d[k / 2] * a.d[k / 2];
    } else {
#pragma unroll
      for (int i = i0; i <= i1; i++) ap += (uint64_t)a.d[i] * b.d[k - i];
    }
#pragma unroll
    for (int i = i0; i <= i1 && i < k; i++) ar += (uint64_t)m[i] * PD.d[k - i];
    if (k < 13) {
      m[k] = (((uint32_t)ap + (uint32_t)ar) * PINV30) & M30;
      ar += (uint64_t)m[k] * PD.d[0];
    }
    ar += (uint32_t)ap & M30;  // for k < 13 the column is now 0 mod 2^30
    if (k >= 13) r.d[k - 13] = (uint32_t)ar & M30;
    cp = ap >> 30;
    cr = ar >> 30;
  }
}
LB_HD void mul(d13& r, const d13& a, const d13& b) { mont<false>(r, a, b); }
LB_HD void sqr(d13& r, const d13& a) { mont<true>(r, a, a); }

// r = a^((p-3)/4), 12 limbs in and out in the callers' Montgomery form (R = 2^384), r < p.
// One squaring body and one product body serve the whole function: the odd powers a, a^3, a^5,
// a^7 of the LB_P34_WIN window, the chain and the exit product are steps of one loop whose index
// is uniform, so choosing the multiplier is a scalar branch and 13 moves.
LB_HD void pow_p34(uint32_t* r, const uint32_t* a) {
  enum { T1 = 0, T3 = 1, T5 = 2, T7 = 3, AUX = 4, NONE = 15 };
  d13 t1, t3, t5, t7, aux, acc;  // aux: a^2 while the odd powers are built, then the exit constant
  enter(t1, a);
  acc = aux = t3 = t5 = t7 = t1;
#pragma unroll 1
  for (int k = -4; k <= LB_P34_WIN_STEPS; k++) {
    // step word as in LB_P34_WIN: squarings << 4 | multiplier
    uint32_t st;
    if (k == -4) st = (1u << 4) | NONE;        // a^2
    else if (k == -3) st = T1;                 // a^3 = a^2 a
    else if (k < 0) st = AUX;                  // a^5, a^7
    else if (k == 0) st = NONE;                // the window program's first entry is a load
    else if (k < LB_P34_WIN_STEPS) st = LB_P34_WIN[k];
    else st = AUX;                             // 2^390 -> 2^384 form
#pragma unroll 1
    for (uint32_t q = st >> 4; q > 0; q--) {
      LB_COUNT_SQR();
      sqr(acc, acc);
    }
    d13 m = t1;
    bool product = true;
    switch (st & 15) {
      case T1: break;
      case T3: m = t3; break;
      case T5: m = t5; break;
      case T7: m = t7; break;
      case AUX: m = aux; break;
      default: product = false; break;
    }
    if (product) {
      if (k < LB_P34_WIN_STEPS) LB_COUNT_MUL();
      mul(acc, acc, m);
    }
    if (k == -4) aux = acc;
    else if (k == -3) t3 = acc;
    else if (k == -2) t5 = acc;
    else if (k == -1) t7 = acc;
    else if (k == 0) {
      aux = EXIT;
      switch (LB_P34_WIN[0] & 15) {
        case 0: acc = t1; break;
        case 1: acc = t3; break;
        case 2: acc = t5; break;
        default: acc = t7; break;
      }
    }
  }
  leave(r, acc);
}

}  // namespace pw
}  // namespace lb
