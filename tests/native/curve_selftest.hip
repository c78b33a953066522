// Test-only HIP library: the group law, scalar ladders, endomorphisms, subgroup
// checks and ZCash encodings of bls_curve.h, one point per lane, on G1 (g = 1,
// field element F = 12 words) and G2 (g = 2, F = 24 words).  Points travel as raw
// little-endian 32-bit limbs in Montgomery form: a Jacobian point is X | Y | Z
// (3 F words; Z = 0 is infinity, whatever X and Y hold), an affine point is
// x | y | inf (2 F + 1 words).  tests/test_gpu_curve.py normalises in Python
// (x = X / Z^2, y = Y / Z^3) and compares with the pure-Python oracle, so no
// routine under test sits in the I/O path.  Never linked into the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bls_curve.h"

namespace {
using namespace lb;

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
template <class F>
LB_DEV void ld_jac(jac<F>& p, const uint32_t* w) {
  ldw(p.X, w);
  ldw(p.Y, w + sizeof(F) / 4);
  ldw(p.Z, w + 2 * (sizeof(F) / 4));
}
template <class F>
LB_DEV void st_jac(uint32_t* w, const jac<F>& p) {
  stw(w, p.X);
  stw(w + sizeof(F) / 4, p.Y);
  stw(w + 2 * (sizeof(F) / 4), p.Z);
}
template <class F>
LB_DEV void ld_aff(aff<F>& p, const uint32_t* w) {
  ldw(p.x, w);
  ldw(p.y, w + sizeof(F) / 4);
  p.inf = w[2 * (sizeof(F) / 4)] != 0;
}
template <class F>
LB_DEV void st_aff(uint32_t* w, const aff<F>& p) {
  stw(w, p.x);
  stw(w + sizeof(F) / 4, p.y);
  w[2 * (sizeof(F) / 4)] = p.inf ? 1u : 0u;
}

// the launch bound of the product's tower kernels (TPB = 64, one wave per SIMD)
#define LBT_KERNEL __global__ void __launch_bounds__(64, 1)

enum {
  C_DBL = 0, C_ADD, C_ADD_AFF, C_NEG, C_EQ, C_TO_AFF,
  C_PAIR_TO_AFF = 10,
  C_MUL_U64 = 20, C_MUL_GLV, C_MUL_XABS,
  C_PSI = 30, C_GLV_ENDO, C_IN_SUBGROUP,
  C_SERIALIZE = 40, C_COMPRESS,
};

LB_DEV void endo(g1j& r, const g1j& p) { g1_glv_endo(r, p); }
LB_DEV void endo(g2j& r, const g2j& p) { g2_glv_endo(r, p); }
LB_DEV bool in_subgroup(const g1j& p) { return g1_in_subgroup(p); }
LB_DEV bool in_subgroup(const g2j& p) { return g2_in_subgroup(p); }
LB_DEV void glv(g1j& r, const g1j& p, uint64_t raw) { jac_mul_glv(r, p, LB_G1_BETA, LB_G1_BETA2, raw); }
LB_DEV void glv(g2j& r, const g2j& p, uint64_t raw) { jac_mul_glv(r, p, LB_G2_OMEGA, LB_G2_OMEGA2, raw); }
LB_DEV void psi(g1j& r, const g1j& p) { r = p; }  // (G2 only; the host entry rejects g = 1)
LB_DEV void psi(g2j& r, const g2j& p) { g2_psi(r, p); }
LB_DEV void serialize(uint8_t* o, const g1a& a) { g1_serialize(o, a); }
LB_DEV void serialize(uint8_t* o, const g2a& a) { g2_serialize(o, a); }
LB_DEV void compress(uint8_t* o, const g1a& a) { g1_compress(o, a); }
LB_DEV void compress(uint8_t* o, const g2a& a) { g2_compress(o, a); }

// var: 0 = result in a distinct object, 1 = in place (r is p), the form the ladders use;
// for C_ADD, 2 = r is q and 3 = q is p (the same object)
template <class F>
LBT_KERNEL k_law(int op, int var, uint32_t n, uint32_t wa, uint32_t wb, uint32_t wo, const uint32_t* __restrict__ a,
                 const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a += (size_t)wa * i;
  b += (size_t)wb * i;
  out += (size_t)wo * i;
  jac<F> p, q, r;
  ld_jac(p, a);
  switch (op) {
    case C_DBL:
      if (var) { jac_dbl(p, p); r = p; } else { jac_dbl(r, p); }
      break;
    case C_ADD:
      ld_jac(q, b);
      if (var == 1) { jac_add(p, p, q); r = p; }
      else if (var == 2) { jac_add(q, p, q); r = q; }
      else if (var == 3) { jac_add(r, p, p); }
      else { jac_add(r, p, q); }
      break;
    case C_ADD_AFF: {
      aff<F> qa;
      ld_aff(qa, b);
      if (var) { jac_add_aff(p, p, qa); r = p; } else { jac_add_aff(r, p, qa); }
      break;
    }
    case C_NEG:
      if (var) { jac_neg(p, p); r = p; } else { jac_neg(r, p); }
      break;
    case C_EQ:
      ld_jac(q, b);
      out[0] = (var == 3 ? jac_eq(p, p) : jac_eq(p, q)) ? 1u : 0u;
      return;
    case C_TO_AFF: {
      aff<F> ra;
      jac_to_aff(ra, p);
      st_aff(out, ra);
      return;
    }
    default: return;
  }
  st_jac(out, r);
}

// a = g1j | g2j -> g1a | g2a
LBT_KERNEL k_pair(uint32_t n, const uint32_t* __restrict__ a, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  g1j p;
  g2j q;
  ld_jac(p, a + (size_t)108 * i);
  ld_jac(q, a + (size_t)108 * i + 36);
  g1a pa;
  g2a qa;
  jac_pair_to_aff(pa, qa, p, q);
  st_aff(out + (size_t)74 * i, pa);
  st_aff(out + (size_t)74 * i + 25, qa);
}

template <class F>
LBT_KERNEL k_mul(int op, int var, uint32_t n, uint32_t w, const uint32_t* __restrict__ a, const uint64_t* __restrict__ k,
                 uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  jac<F> p, r;
  ld_jac(p, a + (size_t)w * i);
  switch (op) {
    case C_MUL_U64:
      if (var) { jac_mul_u64(p, p, k[i]); r = p; } else { jac_mul_u64(r, p, k[i]); }
      break;
    case C_MUL_GLV:
      if (var) { glv(p, p, k[i]); r = p; } else { glv(r, p, k[i]); }
      break;
    case C_MUL_XABS:
      if (var) { jac_mul_xabs(p, p); r = p; } else { jac_mul_xabs(r, p); }
      break;
    default: return;
  }
  st_jac(out + (size_t)w * i, r);
}

template <class F>
LBT_KERNEL k_endo(int op, int var, uint32_t n, uint32_t w, uint32_t wo, const uint32_t* __restrict__ a,
                  uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  jac<F> p, r;
  ld_jac(p, a + (size_t)w * i);
  out += (size_t)wo * i;
  switch (op) {
    case C_PSI:
      if (var) { psi(p, p); r = p; } else { psi(r, p); }
      break;
    case C_GLV_ENDO:
      if (var) { endo(p, p); r = p; } else { endo(r, p); }
      break;
    case C_IN_SUBGROUP: out[0] = in_subgroup(p) ? 1u : 0u; return;
    default: return;
  }
  st_jac(out, r);
}

// a = affine point -> bytes (packed four to a word, little-endian)
template <class F>
LBT_KERNEL k_ser(int op, uint32_t n, uint32_t wa, uint32_t wo, const uint32_t* __restrict__ a, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  aff<F> p;
  ld_aff(p, a + (size_t)wa * i);
  uint8_t bytes[8 * sizeof(F) / 4];  // 96 (G1) or 192 (G2)
  for (uint32_t j = 0; j < sizeof(bytes); j++) bytes[j] = 0;
  if (op == C_SERIALIZE) serialize(bytes, p); else compress(bytes, p);
  out += (size_t)wo * i;
  for (uint32_t j = 0; j < wo; j++)
    out[j] = (uint32_t)bytes[4 * j] | ((uint32_t)bytes[4 * j + 1] << 8) | ((uint32_t)bytes[4 * j + 2] << 16) |
             ((uint32_t)bytes[4 * j + 3] << 24);
}

// words per record (a, b, out) and whether the op takes one 64-bit scalar per record
bool widths(int op, int g, uint32_t w[3], bool& scalar) {
  if (g != 1 && g != 2) return false;
  const uint32_t F = 12u * g, J = 3 * F, A = 2 * F + 1;
  scalar = false;
  w[1] = 0;
  switch (op) {
    case C_DBL: case C_NEG: case C_MUL_XABS: case C_GLV_ENDO: w[0] = w[2] = J; break;
    case C_PSI: if (g != 2) return false; w[0] = w[2] = J; break;
    case C_ADD: w[0] = w[1] = w[2] = J; break;
    case C_ADD_AFF: w[0] = w[2] = J; w[1] = A; break;
    case C_EQ: w[0] = w[1] = J; w[2] = 1; break;
    case C_TO_AFF: w[0] = J; w[2] = A; break;
    case C_PAIR_TO_AFF: w[0] = 108; w[2] = 74; break;
    case C_MUL_U64: case C_MUL_GLV: w[0] = w[2] = J; scalar = true; break;
    case C_IN_SUBGROUP: w[0] = J; w[2] = 1; break;
    case C_SERIALIZE: w[0] = A; w[2] = 2 * F; break;
    case C_COMPRESS: w[0] = A; w[2] = F; break;
    default: return false;
  }
  return true;
}

template <class F>
void launch(int op, int var, uint32_t n, const uint32_t w[3], const uint32_t* a, const uint32_t* b, const uint64_t* k,
            uint32_t* out) {
  const dim3 grid((n + 63) / 64), block(64);
  if (op < C_PAIR_TO_AFF)
    hipLaunchKernelGGL(k_law<F>, grid, block, 0, 0, op, var, n, w[0], w[1], w[2], a, b, out);
  else if (op == C_PAIR_TO_AFF)
    hipLaunchKernelGGL(k_pair, grid, block, 0, 0, n, a, out);
  else if (op < C_PSI)
    hipLaunchKernelGGL(k_mul<F>, grid, block, 0, 0, op, var, n, w[0], a, k, out);
  else if (op < C_SERIALIZE)
    hipLaunchKernelGGL(k_endo<F>, grid, block, 0, 0, op, var, n, w[0], w[2], a, out);
  else
    hipLaunchKernelGGL(k_ser<F>, grid, block, 0, 0, op, n, w[0], w[2], a, out);
}
}  // namespace

// Words per record (a, b, out) of op on group g; 0 = ok, 1 = unknown op.
extern "C" int lbt_curve_op_widths(int op, int g, uint32_t* w) {
  bool scalar;
  return widths(op, g, w, scalar) ? 0 : 1;
}

// Host-buffer entry: n records of a (and of b, and one scalar each in k, where the op takes
// them), n records out.  0 = ok.
extern "C" int lbt_curve_op(int op, int g, int var, uint32_t n, const uint32_t* a, const uint32_t* b, const uint64_t* k,
                            uint32_t* out) {
  uint32_t w[3];
  bool scalar;
  if (!widths(op, g, w, scalar) || n == 0 || !a || !out || (w[1] && !b) || (scalar && !k)) return 5;
  uint32_t *da = nullptr, *db = nullptr, *dout = nullptr;
  uint64_t* dk = nullptr;
  if (hipMalloc(&da, (size_t)n * w[0] * 4) != hipSuccess || hipMalloc(&db, (size_t)n * (w[1] ? w[1] : 1) * 4) != hipSuccess ||
      hipMalloc(&dk, (size_t)n * 8) != hipSuccess || hipMalloc(&dout, (size_t)n * w[2] * 4) != hipSuccess)
    return 1;
  int rc = 0;
  if (hipMemcpy(da, a, (size_t)n * w[0] * 4, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
  if (!rc && w[1] && hipMemcpy(db, b, (size_t)n * w[1] * 4, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
  if (!rc && scalar && hipMemcpy(dk, k, (size_t)n * 8, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
  if (!rc && hipMemset(dout, 0, (size_t)n * w[2] * 4) != hipSuccess) rc = 2;
  if (!rc) {
    if (g == 1) launch<fp>(op, var, n, w, da, db, dk, dout); else launch<fp2>(op, var, n, w, da, db, dk, dout);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 3;
  }
  if (!rc && hipMemcpy(out, dout, (size_t)n * w[2] * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = 4;
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dk);
  (void)hipFree(dout);
  return rc;
}
