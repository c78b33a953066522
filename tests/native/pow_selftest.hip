// Test-only HIP library: the resident exponentiation (bls_fp_pow.h) one primitive at a time, one
// element per lane, so that a disagreement between the gfx950 build and Python integers is
// pinned to one operation.  tests/test_gpu_pow_cols.py feeds the cases of
// tests/pow_cols_cases.py.  Never linked into the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bls_field.h"
#include "bls_fp_pow.h"

namespace {
using namespace lb;

// the resident exponentiation out of line, as fp_pow_p34_r holds it
__device__ __noinline__ fp_ret pow_cols_r(LB_FP_PARAMS(x)) {
  const uint32_t a[12] = {x0, x1, x2, x3, x4, x5, x6, x7, x8, x9, x10, x11};
  uint32_t r[12];
  pw::pow_p34(r, a);
  return fp_ret{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11]};
}

// op 0: enter (a: 12 limbs)            -> 13 digits
// op 1: leave (a: 13 digits, < 2p)     -> 12 limbs
// op 2: resident sqr (a: 13 digits)    -> 13 digits (in place, as the chain calls it)
// op 3: resident mul (a, b: 13 digits) -> 13 digits (in place)
// op 4: pw::pow_p34 (a: 12 limbs)      -> 12 limbs
// op 5: fp_pow_p34 (a: 12 limbs)       -> 12 limbs (this build's LB_POW_COLS)
// words per record; which 0: a, 1: b, 2: out
__host__ __device__ constexpr uint32_t width(int op, int which) {
  if (which == 1) return op == 3 ? 13 : 0;
  if (which == 0) return (op >= 1 && op <= 3) ? 13 : 12;
  return (op == 0 || op == 2 || op == 3) ? 13 : 12;
}

__global__ void __launch_bounds__(64, 2) k_pow_selftest(int op, uint32_t n, const uint32_t* __restrict__ a,
                                                        const uint32_t* __restrict__ b, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a += (size_t)width(op, 0) * i;
  b += (size_t)width(op, 1) * i;
  out += (size_t)width(op, 2) * i;
  if (op == 0) {
    uint32_t x[12];
    for (int j = 0; j < 12; j++) x[j] = a[j];
    pw::d13 d;
    pw::enter(d, x);
    for (int j = 0; j < 13; j++) out[j] = d.d[j];
  } else if (op == 1) {
    pw::d13 d;
    for (int j = 0; j < 13; j++) d.d[j] = a[j];
    uint32_t r[12];
    pw::leave(r, d);
    for (int j = 0; j < 12; j++) out[j] = r[j];
  } else if (op == 2 || op == 3) {
    pw::d13 x, y;
    for (int j = 0; j < 13; j++) x.d[j] = a[j];
    if (op == 3) {
      for (int j = 0; j < 13; j++) y.d[j] = b[j];
      pw::mul(x, x, y);
    } else {
      pw::sqr(x, x);
    }
    for (int j = 0; j < 13; j++) out[j] = x.d[j];
  } else {
    fp x, r;
    for (int j = 0; j < 12; j++) x.l[j] = a[j];
    if (op == 4) fp_unret(r, pow_cols_r(LB_FP_ARGS(x))); else fp_pow_p34(r, x);
    for (int j = 0; j < 12; j++) out[j] = r.l[j];
  }
}
}  // namespace

extern "C" int lbt_pow_cols_switch() { return LB_POW_COLS; }

// Host-buffer entry: copies in, runs op over n elements (one launch), copies out.  0 = ok.
extern "C" int lbt_pow_op(int op, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  if (op < 0 || op > 5 || n == 0 || !a || !out || (op == 3 && !b)) return 5;
  const size_t wa = width(op, 0), wb = width(op, 1), wo = width(op, 2);
  uint32_t *da = nullptr, *db = nullptr, *dout = nullptr;
  if (hipMalloc(&da, n * wa * 4) != hipSuccess || hipMalloc(&db, n * (wb ? wb : 1) * 4) != hipSuccess ||
      hipMalloc(&dout, n * wo * 4) != hipSuccess)
    return 1;
  int rc = 0;
  if (hipMemcpy(da, a, n * wa * 4, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
  if (!rc && wb && hipMemcpy(db, b, n * wb * 4, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
  if (!rc && hipMemset(dout, 0, n * wo * 4) != hipSuccess) rc = 2;
  if (!rc) {
    hipLaunchKernelGGL(k_pow_selftest, dim3((n + 63) / 64), dim3(64), 0, 0, op, n, da, db, dout);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 3;
  }
  if (!rc && hipMemcpy(out, dout, n * wo * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = 4;
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  return rc;
}
