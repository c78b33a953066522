// Test-only HIP library: the field primitives behind the lazy-reduction Fp2
// product and the register-window exponentiation, one element per lane, raw
// little-endian 32-bit limbs in Montgomery form.  tests/test_gpu_field.py feeds
// edge cases (0, 1, p - 1, limbs of all ones, 2p - 1 where the bound allows)
// and checks every output against Python big integers.  A second entry point
// (lbt_field_op2, below) covers the rest of the one-lane tower, Fp ... Fp12, in
// the aliasing forms the product calls.  Never linked into the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bls_field.h"

namespace {
using namespace lb;

LB_DEV void load(fp& a, const uint32_t* p) {
#pragma unroll
  for (int j = 0; j < 12; j++) a.l[j] = p[j];
}
LB_DEV void store(uint32_t* p, const fp& a) {
#pragma unroll
  for (int j = 0; j < 12; j++) p[j] = a.l[j];
}

// op 0: fp2_mul (a, b: 24 limbs each) -> 24 limbs
// op 1: fp_mulw (a, b: 12 limbs)      -> 24 limbs (double width)
// op 2: fp_redc (a: 24 limbs)         -> 12 limbs
// op 3: fp_pow_p34 (a: 12 limbs)      -> 12 limbs
// op 4: fp_mul (a, b: 12 limbs)       -> 12 limbs
// op 5: fp_sqr (a: 12 limbs)          -> 12 limbs
__global__ void k_selftest(int op, uint32_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                           uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (op == 0) {
    fp2 x, y, r;
    load(x.c0, a + 24 * i);
    load(x.c1, a + 24 * i + 12);
    load(y.c0, b + 24 * i);
    load(y.c1, b + 24 * i + 12);
    fp2_mul(r, x, y);
    store(out + 24 * i, r.c0);
    store(out + 24 * i + 12, r.c1);
  } else if (op == 1) {
    fp x, y;
    load(x, a + 12 * i);
    load(y, b + 12 * i);
    uint32_t w[24];
    fp_mulw(w, x, y);
    for (int j = 0; j < 24; j++) out[24 * i + j] = w[j];
  } else if (op == 2) {
    uint32_t w[24];
    for (int j = 0; j < 24; j++) w[j] = a[24 * i + j];
    fp r;
    fp_redc(r, w);
    store(out + 12 * i, r);
  } else if (op == 3) {
    fp x, r;
    load(x, a + 12 * i);
    fp_pow_p34(r, x);
    store(out + 12 * i, r);
  } else if (op == 4) {
    fp x, y, r;
    load(x, a + 12 * i);
    load(y, b + 12 * i);
    fp_mul(r, x, y);
    store(out + 12 * i, r);
  } else {
    fp x, r;
    load(x, a + 12 * i);
    fp_sqr(r, x);
    store(out + 12 * i, r);
  }
}

// ---- second entry point: the rest of the tower, one __global__ per family ----
// Records are whole elements (fp = 12 words, fp2 = 24, fp6 = 72, fp12 = 144).
// `var` selects the aliasing form the routine is called in:
//   0: r, a, b distinct objects      1: r is a        2: r is b
//   3: a is b (the same object; b's record is ignored)     4: r is a is b
// (unary routines: 0 distinct, 1 in place).
template <class T>
LB_DEV void ldw(T& x, const uint32_t* p) {
  uint32_t* q = reinterpret_cast<uint32_t*>(&x);
#pragma unroll
  for (uint32_t j = 0; j < sizeof(T) / 4; j++) q[j] = p[j];
}
template <class T>
LB_DEV void stw(uint32_t* p, const T& x) {
  const uint32_t* q = reinterpret_cast<const uint32_t*>(&x);
#pragma unroll
  for (uint32_t j = 0; j < sizeof(T) / 4; j++) p[j] = q[j];
}
template <class T, class Op>
LB_DEV void bin(int var, T& r, T& x, T& y, Op op) {
  switch (var) {
    case 0: op(r, x, y); break;
    case 1: op(x, x, y); r = x; break;
    case 2: op(y, x, y); r = y; break;
    case 3: op(r, x, x); break;
    default: op(x, x, x); r = x; break;
  }
}
template <class T, class Op>
LB_DEV void un(int var, T& r, T& x, Op op) {
  if (var) {
    op(x, x);
    r = x;
  } else {
    op(r, x);
  }
}
#define LBT_BIN(T, f) [](T& r, const T& a, const T& b) { f(r, a, b); }
#define LBT_UN(T, f) [](T& r, const T& a) { f(r, a); }
// the launch bound of the product's tower kernels (TPB = 64, one wave per SIMD)
#define LBT_KERNEL __global__ void __launch_bounds__(64, 1)

enum {
  F_ADD = 100, F_SUB, F_NEG, F_DBL, F_MUL3, F_ADD2_PLAIN, F_INV, F_SQRT, F_IS_SQUARE, F_LEX, F_PARITY, F_TO_MONT,
  F_FROM_MONT, F_FROM_BE48, F_TO_BE48, F_MUL, F_SQR,
  F2_ADD = 200, F2_SUB, F2_SUBADD, F2_DBL, F2_NEG, F2_CONJ, F2_MUL_XI, F2_SQR, F2_MUL_FP, F2_MUL3, F2_INV, F2_SGN0,
  F2_LEX, F2_SQRT, FW_KCOMBINE, F2_MUL,
  F6_MUL = 300, F6_MUL_01, F6_MUL_1, F6_MUL_12, F6_MUL_V, F6_INV,
  F12_MUL = 400, F12_SQR, F12_CONJ, F12_INV,
  F12_MUL_LINE = 450, F12_LINE_LINE, F12_FROB1, F12_FROB2, F12_FROB3, F12_CYC_SQR, F12_IS_ONE,
};

LBT_KERNEL k_fp(int op, int var, uint32_t n, uint32_t wa, uint32_t wb, uint32_t wo, const uint32_t* __restrict__ a,
                const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a += (size_t)wa * i;
  b += (size_t)wb * i;
  out += (size_t)wo * i;
  fp x, y, r;
  fp_zero(r);
  fp_zero(y);
  ldw(x, a);
  if (wb >= 12) ldw(y, b);
  bool flag = false, has_flag = false;
  switch (op) {
    case F_ADD: bin(var, r, x, y, LBT_BIN(fp, fp_add)); break;
    case F_SUB: bin(var, r, x, y, LBT_BIN(fp, fp_sub)); break;
    case F_MUL: bin(var, r, x, y, LBT_BIN(fp, fp_mul)); break;
    case F_NEG: un(var, r, x, LBT_UN(fp, fp_neg)); break;
    case F_DBL: un(var, r, x, LBT_UN(fp, fp_dbl)); break;
    case F_MUL3: un(var, r, x, LBT_UN(fp, fp_mul3)); break;
    case F_INV: un(var, r, x, LBT_UN(fp, fp_inv)); break;
    case F_SQR: un(var, r, x, LBT_UN(fp, fp_sqr)); break;
    case F_TO_MONT: un(var, r, x, LBT_UN(fp, fp_to_mont)); break;
    case F_FROM_MONT: un(var, r, x, LBT_UN(fp, fp_from_mont)); break;
    case F_ADD2_PLAIN: {
      fp a1, b1, s, t;
      ldw(a1, a + 12);
      ldw(b1, b + 12);
      if (var == 3) fp_add2_plain_ps(s, t, x, x, y, y); else fp_add2_plain_ps(s, t, x, a1, y, b1);
      stw(out, s);
      stw(out + 12, t);
      return;
    }
    case F_SQRT:
      if (var) { flag = fp_sqrt(x, x); r = x; } else { flag = fp_sqrt(r, x); }
      has_flag = true;
      break;
    case F_IS_SQUARE: out[0] = fp_is_square(x) ? 1u : 0u; return;
    case F_LEX: out[0] = fp_lex_largest(x) ? 1u : 0u; return;
    case F_PARITY: out[0] = fp_parity(x); return;
    case F_FROM_BE48: {
      uint8_t bytes[48];
      for (int j = 0; j < 48; j++) bytes[j] = (uint8_t)(a[j >> 2] >> (8 * (j & 3)));
      flag = fp_from_be48_raw(r, bytes);
      has_flag = true;
      break;
    }
    case F_TO_BE48: {
      uint8_t bytes[48];
      fp_to_be48_raw(bytes, x);
      for (int j = 0; j < 12; j++)
        out[j] = (uint32_t)bytes[4 * j] | ((uint32_t)bytes[4 * j + 1] << 8) | ((uint32_t)bytes[4 * j + 2] << 16) |
                 ((uint32_t)bytes[4 * j + 3] << 24);
      return;
    }
    default: return;
  }
  stw(out, r);
  if (has_flag) out[12] = flag ? 1u : 0u;
}

LBT_KERNEL k_fp2(int op, int var, uint32_t n, uint32_t wa, uint32_t wb, uint32_t wo, const uint32_t* __restrict__ a,
                 const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a += (size_t)wa * i;
  b += (size_t)wb * i;
  out += (size_t)wo * i;
  if (op == FW_KCOMBINE) {  // a = T0 | T1, b = T2 -> T0', T2'
    uint32_t t0[24], t1[24], t2[24];
    for (int j = 0; j < 24; j++) {
      t0[j] = a[j];
      t1[j] = a[24 + j];
      t2[j] = b[j];
    }
    fpw_kcombine_ps(t0, t1, t2);
    for (int j = 0; j < 24; j++) {
      out[j] = t0[j];
      out[24 + j] = t2[j];
    }
    return;
  }
  fp2 x, y, r;
  fp2_zero(r);
  fp2_zero(y);
  ldw(x, a);
  if (wb >= 24) ldw(y, b);
  switch (op) {
    case F2_ADD: bin(var, r, x, y, LBT_BIN(fp2, fp2_add)); break;
    case F2_SUB: bin(var, r, x, y, LBT_BIN(fp2, fp2_sub)); break;
    case F2_SUBADD: bin(var, r, x, y, LBT_BIN(fp2, fp2_subadd_ps)); break;
    case F2_MUL: bin(var, r, x, y, LBT_BIN(fp2, fp2_mul)); break;
    case F2_DBL: un(var, r, x, LBT_UN(fp2, fp2_dbl)); break;
    case F2_NEG: un(var, r, x, LBT_UN(fp2, fp2_neg)); break;
    case F2_CONJ: un(var, r, x, LBT_UN(fp2, fp2_conj)); break;
    case F2_MUL_XI: un(var, r, x, LBT_UN(fp2, fp2_mul_xi)); break;
    case F2_SQR: un(var, r, x, LBT_UN(fp2, fp2_sqr)); break;
    case F2_MUL3: un(var, r, x, LBT_UN(fp2, fp2_mul3)); break;
    case F2_INV: un(var, r, x, LBT_UN(fp2, fp2_inv)); break;
    case F2_MUL_FP: {
      fp k;
      ldw(k, b);
      if (var) { fp2_mul_fp(x, x, k); r = x; } else { fp2_mul_fp(r, x, k); }
      break;
    }
    case F2_SGN0: out[0] = fp2_sgn0(x); return;
    case F2_LEX: out[0] = fp2_lex_largest(x) ? 1u : 0u; return;
    case F2_SQRT: {
      bool ok;
      if (var) { ok = fp2_sqrt(x, x); r = x; } else { ok = fp2_sqrt(r, x); }
      if (!ok) fp2_zero(r);
      out[24] = ok ? 1u : 0u;
      break;
    }
    default: return;
  }
  stw(out, r);
}

LBT_KERNEL k_fp6(int op, int var, uint32_t n, uint32_t wa, uint32_t wb, uint32_t wo, const uint32_t* __restrict__ a,
                 const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a += (size_t)wa * i;
  b += (size_t)wb * i;
  out += (size_t)wo * i;
  fp6 x, r;
  ldw(x, a);
  switch (op) {
    case F6_MUL: {
      fp6 y;
      ldw(y, b);
      bin(var, r, x, y, LBT_BIN(fp6, fp6_mul));
      break;
    }
    case F6_MUL_01: {
      fp2 b0, b1;
      ldw(b0, b);
      ldw(b1, b + 24);
      if (var) { fp6_mul_01(x, x, b0, b1); r = x; } else { fp6_mul_01(r, x, b0, b1); }
      break;
    }
    case F6_MUL_1: {
      fp2 b1;
      ldw(b1, b);
      if (var) { fp6_mul_1(x, x, b1); r = x; } else { fp6_mul_1(r, x, b1); }
      break;
    }
    case F6_MUL_12: {
      fp2 y1, y2;
      ldw(y1, b);
      ldw(y2, b + 24);
      if (var) { fp6_mul_12(x, x, y1, y2); r = x; } else { fp6_mul_12(r, x, y1, y2); }
      break;
    }
    case F6_MUL_V: un(var, r, x, LBT_UN(fp6, fp6_mul_v)); break;
    case F6_INV: un(var, r, x, LBT_UN(fp6, fp6_inv)); break;
    default: return;
  }
  stw(out, r);
}

LBT_KERNEL k_fp12(int op, int var, uint32_t n, uint32_t wa, uint32_t wb, uint32_t wo, const uint32_t* __restrict__ a,
                  const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a += (size_t)wa * i;
  b += (size_t)wb * i;
  out += (size_t)wo * i;
  fp12 x, r;
  ldw(x, a);
  switch (op) {
    case F12_MUL: {
      fp12 y;
      ldw(y, b);
      bin(var, r, x, y, LBT_BIN(fp12, fp12_mul));
      break;
    }
    case F12_SQR: un(var, r, x, LBT_UN(fp12, fp12_sqr)); break;
    case F12_CONJ: un(var, r, x, LBT_UN(fp12, fp12_conj)); break;
    case F12_INV: un(var, r, x, LBT_UN(fp12, fp12_inv)); break;
    default: return;
  }
  stw(out, r);
}

// the sparse products, Frobenius and the cyclotomic squaring
LBT_KERNEL k_fp12s(int op, int var, uint32_t n, uint32_t wa, uint32_t wb, uint32_t wo, const uint32_t* __restrict__ a,
                   const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a += (size_t)wa * i;
  b += (size_t)wb * i;
  out += (size_t)wo * i;
  fp12 x, r;
  ldw(x, a);
  switch (op) {
    case F12_MUL_LINE: {
      fp2 l0, l1, l4;
      ldw(l0, b);
      ldw(l1, b + 24);
      ldw(l4, b + 48);
      if (var) { fp12_mul_line(x, x, l0, l1, l4); r = x; } else { fp12_mul_line(r, x, l0, l1, l4); }
      break;
    }
    case F12_LINE_LINE: {  // b = l0 l1 l4 m0 m1 m4
      fp2 l[6];
#pragma unroll
      for (int j = 0; j < 6; j++) ldw(l[j], b + 24 * j);
      fp6 sx;
      fp2 y1, y2;
      line_mul_line(sx, y1, y2, l[0], l[1], l[2], l[3], l[4], l[5]);
      if (var) { fp12_mul_by_sparse2(x, x, sx, y1, y2); r = x; } else { fp12_mul_by_sparse2(r, x, sx, y1, y2); }
      break;
    }
    case F12_FROB1: un(var, r, x, LBT_UN(fp12, fp12_frob1)); break;
    case F12_FROB2: un(var, r, x, LBT_UN(fp12, fp12_frob2)); break;
    case F12_FROB3: un(var, r, x, LBT_UN(fp12, fp12_frob3)); break;
    case F12_CYC_SQR: un(var, r, x, LBT_UN(fp12, fp12_cyc_sqr)); break;
    case F12_IS_ONE: out[0] = fp12_is_one(x) ? 1u : 0u; return;
    default: return;
  }
  stw(out, r);
}

// words per record (a, b, out) of each op of the second entry point; false = unknown op
bool op2_widths(int op, uint32_t w[3]) {
  uint32_t wa, wb = 0, wo;
  switch (op) {
    case F_ADD: case F_SUB: case F_MUL: wa = wb = wo = 12; break;
    case F_NEG: case F_DBL: case F_MUL3: case F_INV: case F_SQR: case F_TO_MONT: case F_FROM_MONT: case F_TO_BE48:
      wa = wo = 12; break;
    case F_ADD2_PLAIN: wa = wb = wo = 24; break;
    case F_SQRT: case F_FROM_BE48: wa = 12; wo = 13; break;
    case F_IS_SQUARE: case F_LEX: case F_PARITY: wa = 12; wo = 1; break;
    case F2_ADD: case F2_SUB: case F2_SUBADD: case F2_MUL: wa = wb = wo = 24; break;
    case F2_DBL: case F2_NEG: case F2_CONJ: case F2_MUL_XI: case F2_SQR: case F2_MUL3: case F2_INV: wa = wo = 24; break;
    case F2_MUL_FP: wa = wo = 24; wb = 12; break;
    case F2_SGN0: case F2_LEX: wa = 24; wo = 1; break;
    case F2_SQRT: wa = 24; wo = 25; break;
    case FW_KCOMBINE: wa = 48; wb = 24; wo = 48; break;
    case F6_MUL: wa = wb = wo = 72; break;
    case F6_MUL_01: case F6_MUL_12: wa = wo = 72; wb = 48; break;
    case F6_MUL_1: wa = wo = 72; wb = 24; break;
    case F6_MUL_V: case F6_INV: wa = wo = 72; break;
    case F12_MUL: wa = wb = wo = 144; break;
    case F12_SQR: case F12_CONJ: case F12_INV: case F12_FROB1: case F12_FROB2: case F12_FROB3: case F12_CYC_SQR:
      wa = wo = 144; break;
    case F12_MUL_LINE: wa = wo = 144; wb = 72; break;
    case F12_LINE_LINE: wa = wo = 144; wb = 144; break;
    case F12_IS_ONE: wa = 144; wo = 1; break;
    default: return false;
  }
  w[0] = wa;
  w[1] = wb;
  w[2] = wo;
  return true;
}
}  // namespace

// Host-buffer entry: copies in, runs op over n elements, copies out.  0 = ok.
extern "C" int lbt_field_op(int op, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  const size_t wa = (op == 0 || op == 2) ? 24 : 12, wb = op == 0 ? 24 : 12;
  const size_t wo = (op == 0 || op == 1) ? 24 : 12;
  uint32_t *da = nullptr, *db = nullptr, *dout = nullptr;
  if (hipMalloc(&da, n * wa * 4) != hipSuccess || hipMalloc(&db, n * wb * 4) != hipSuccess ||
      hipMalloc(&dout, n * wo * 4) != hipSuccess)
    return 1;
  int rc = 0;
  if (hipMemcpy(da, a, n * wa * 4, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
  if (!rc && b && hipMemcpy(db, b, n * wb * 4, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
  if (!rc) {
    hipLaunchKernelGGL(k_selftest, dim3((n + 63) / 64), dim3(64), 0, 0, op, n, da, db, dout);
    if (hipDeviceSynchronize() != hipSuccess) rc = 3;
  }
  if (!rc && hipMemcpy(out, dout, n * wo * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = 4;
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  return rc;
}

// Words per record (a, b, out) of op; 0 = ok, 1 = unknown op.
extern "C" int lbt_field_op2_widths(int op, uint32_t* w) { return op2_widths(op, w) ? 0 : 1; }

// Host-buffer entry for ops >= 100 (the table above): a is n records of w[0] words, b n records of
// w[1] words (may be null when w[1] == 0), out n records of w[2] words.  0 = ok.
extern "C" int lbt_field_op2(int op, int var, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  uint32_t w[3];
  if (!op2_widths(op, w) || n == 0 || !a || !out || (w[1] && !b)) return 5;
  uint32_t *da = nullptr, *db = nullptr, *dout = nullptr;
  if (hipMalloc(&da, (size_t)n * w[0] * 4) != hipSuccess || hipMalloc(&db, (size_t)n * (w[1] ? w[1] : 1) * 4) != hipSuccess ||
      hipMalloc(&dout, (size_t)n * w[2] * 4) != hipSuccess)
    return 1;
  int rc = 0;
  if (hipMemcpy(da, a, (size_t)n * w[0] * 4, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
  if (!rc && w[1] && hipMemcpy(db, b, (size_t)n * w[1] * 4, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
  if (!rc && hipMemset(dout, 0, (size_t)n * w[2] * 4) != hipSuccess) rc = 2;
  if (!rc) {
    const dim3 grid((n + 63) / 64), block(64);
    if (op < 200)
      hipLaunchKernelGGL(k_fp, grid, block, 0, 0, op, var, n, w[0], w[1], w[2], da, db, dout);
    else if (op < 300)
      hipLaunchKernelGGL(k_fp2, grid, block, 0, 0, op, var, n, w[0], w[1], w[2], da, db, dout);
    else if (op < 400)
      hipLaunchKernelGGL(k_fp6, grid, block, 0, 0, op, var, n, w[0], w[1], w[2], da, db, dout);
    else if (op < 450)
      hipLaunchKernelGGL(k_fp12, grid, block, 0, 0, op, var, n, w[0], w[1], w[2], da, db, dout);
    else
      hipLaunchKernelGGL(k_fp12s, grid, block, 0, 0, op, var, n, w[0], w[1], w[2], da, db, dout);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 3;
  }
  if (!rc && hipMemcpy(out, dout, (size_t)n * w[2] * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = 4;
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  return rc;
}
