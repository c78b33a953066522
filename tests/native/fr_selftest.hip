// Test-only HIP library: the one-lane scalar-field arithmetic of bls_fr.h, one element
// per lane.  Elements travel as raw little-endian 32-bit limbs in Montgomery form
// (R = 2^256); tests/test_gpu_fr.py converts in Python and compares with Python
// integers, so no routine under test sits in the I/O path.  The byte codecs take and
// give their 32 bytes as they are.  Never linked into the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bls_fr.h"

namespace {
using namespace lb;

enum {
  F_ADD = 0, F_SUB, F_NEG, F_MUL, F_SQR, F_INV, F_POW,
  F_MUL_ALIAS = 10,  // mul(a, a, a)
  F_ADD_ALIAS,       // add(a, a, b)
  F_SUB_ALIAS,       // sub(b, a, b)
  F_FROM_BE = 20,    // a: 32 bytes -> out limbs, flag = accepted
  F_TO_BE,           // a: limbs -> out 32 bytes
  F_REDUCE,          // a: 8 big-endian words of any 256-bit value -> out limbs (mod r)
};

__global__ void __launch_bounds__(64) k_fr_op(int op, uint32_t n, const uint32_t* __restrict__ a,
                                              const uint32_t* __restrict__ b, uint32_t* __restrict__ out,
                                              uint32_t* __restrict__ flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a += 8 * (size_t)i;
  b += 8 * (size_t)i;
  out += 8 * (size_t)i;
  fr x, y, r;
  fr_set(x, a);
  fr_set(y, b);
  fr_zero(r);
  uint32_t fl = 1;
  switch (op) {
    case F_ADD: fr_add(r, x, y); break;
    case F_SUB: fr_sub(r, x, y); break;
    case F_NEG: fr_neg(r, x); break;
    case F_MUL: fr_mul(r, x, y); break;
    case F_SQR: fr_sqr(r, x); break;
    case F_INV: fr_inv(r, x); break;
    case F_POW: fr_pow(r, x, b); break;
    case F_MUL_ALIAS:
      fr_mul(x, x, x);
      r = x;
      break;
    case F_ADD_ALIAS:
      fr_add(x, x, y);
      r = x;
      break;
    case F_SUB_ALIAS:
      fr_sub(y, x, y);
      r = y;
      break;
    case F_FROM_BE: fl = fr_from_be32(r, reinterpret_cast<const uint8_t*>(a)) ? 1u : 0u; break;
    case F_TO_BE: fr_to_be32(reinterpret_cast<uint8_t*>(out), x); break;
    case F_REDUCE: fr_from_be_words_reduce(r, a); break;
    default: fl = 0xffffffffu; break;
  }
  if (op != F_TO_BE)
    for (int j = 0; j < 8; j++) out[j] = r.l[j];
  flag[i] = fl;
}

}  // namespace

// a, b, out: n x 8 words on the host; flag: n words.  Returns 0, or a hipError_t.
extern "C" int lbt_fr_op(int op, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* out, uint32_t* flag) {
  if (n == 0) return 0;
  const size_t bytes = (size_t)n * 32;
  uint32_t *d_a = nullptr, *d_b = nullptr, *d_o = nullptr, *d_f = nullptr;
  hipError_t e = hipMalloc(&d_a, bytes);
  if (e == hipSuccess) e = hipMalloc(&d_b, bytes);
  if (e == hipSuccess) e = hipMalloc(&d_o, bytes);
  if (e == hipSuccess) e = hipMalloc(&d_f, (size_t)n * 4);
  if (e == hipSuccess) e = hipMemcpy(d_a, a, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_b, b, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_o, 0, bytes);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_fr_op, dim3((n + 63) / 64), dim3(64), 0, 0, op, n, (const uint32_t*)d_a,
                       (const uint32_t*)d_b, d_o, d_f);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_o, bytes, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(flag, d_f, (size_t)n * 4, hipMemcpyDeviceToHost);
  (void)hipFree(d_a);
  (void)hipFree(d_b);
  (void)hipFree(d_o);
  (void)hipFree(d_f);
  return (int)e;
}
