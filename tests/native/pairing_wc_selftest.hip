// Test-only HIP library, wave-cooperative half: wc_apply over the eight generated
// programs, wc_exp_x, wc_final_exp, wc_miller_from_lines, wc_is_one and the slot
// helpers of bls_wc12.h, one case per 64-lane workgroup with wc_smem in LDS, as the
// product's tail kernels run them.  (The one-lane half is pairing_selftest.hip; both
// link into libpairing_selftest.so.)  An Fp12 travels as its 12 coefficients in
// tower order, raw little-endian 32-bit Montgomery limbs (144 words).
// tests/test_gpu_pairing.py converts in Python, so no routine under test sits in the
// I/O path.  Never linked into the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bls_kernels.h"
#include "bls_wc12.h"

namespace {
using namespace lb;

#define LBT_KERNEL __global__ void __launch_bounds__(TPB, LB_W_TAIL)

enum { W_APPLY = 0, W_SLOTS, W_IS_ONE, W_EXP_X, W_FINAL_EXP };

// 12 coefficients of 12 words into / out of a slot (lanes 0..11), without wc_load12 / wc_store
LB_DEV void slot_in(wc_smem& S, int slot, const uint32_t* w) {
  if (threadIdx.x < 12) {
    fp v;
#pragma unroll
    for (int j = 0; j < 12; j++) v.l[j] = w[12 * threadIdx.x + j];
    S.slot[slot][threadIdx.x] = v;
  }
  __syncthreads();
}
LB_DEV void slot_out(uint32_t* w, const wc_smem& S, int slot) {
  if (threadIdx.x < 12) {
    const fp v = S.slot[slot][threadIdx.x];
#pragma unroll
    for (int j = 0; j < 12; j++) w[12 * threadIdx.x + j] = v.l[j];
  }
}

// One case per workgroup.  a, b: 144 words per case; out: 145 (Fp12 | flag).
//   W_APPLY    wop = the program.  Operands in WC_A and WC_B (all twelve coefficients of
//              b are loaded, also for LB_WC_LINE), result in WC_C unless it aliases.
//              var 0: dst distinct; 1: dst == a; 2: dst == b; 3: b is a (one slot);
//              4: the Frobenius programs with b from the host instead of the gamma slot
//              (var 0, 1 of a Frobenius program read WC_G1..3 as wc_init_gammas left them).
//              The square programs and LB_WC_CONJ are called as the product calls them,
//              with b == a.
//   W_SLOTS    var 0: wc_load12 -> wc_store; 1: wc_load12 -> wc_copy -> wc_store;
//              2: wc_set_one -> wc_store
//   W_IS_ONE   flag = wc_is_one(a)
//   W_EXP_X    var 0: dst != src; 1: dst == src
//   W_FINAL_EXP  var 0: dst != src (k_gt_check's form); 1: dst == src (k_tail's);
//              flag = wc_is_one(result)
LBT_KERNEL k_wc(int op, int wop, int var, uint32_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                uint32_t* __restrict__ out) {
  __shared__ wc_smem S;
  const uint32_t i = blockIdx.x;
  if (i >= n) return;
  a += (size_t)144 * i;
  b += (size_t)144 * i;
  out += (size_t)145 * i;
  wc_init_tables(S);
  wc_init_gammas(S);
  int res = WC_C;
  uint32_t flag = 0;
  switch (op) {
    case W_APPLY: {
      slot_in(S, WC_A, a);
      slot_in(S, WC_B, b);
      const bool frob = wop == LB_WC_FROB1 || wop == LB_WC_FROB2 || wop == LB_WC_FROB3;
      const bool unary = wop == LB_WC_SQR || wop == LB_WC_CYC || wop == LB_WC_CONJ;
      int sb = WC_B;
      if (unary || var == 3) sb = WC_A;
      if (frob && var != 4) sb = wop == LB_WC_FROB1 ? WC_G1 : wop == LB_WC_FROB2 ? WC_G2 : WC_G3;
      if (var == 1) res = WC_A;
      if (var == 2) res = WC_B;
      wc_apply(S, wop, res, WC_A, sb);
      break;
    }
    case W_SLOTS: {
      fp12 v, r;
      if (var == 2) {
        wc_set_one(S, WC_B);
      } else {
        fp* pv = &v.c0.c0.c0;
        for (int j = 0; j < 12; j++)
          for (int k = 0; k < 12; k++) pv[j].l[k] = a[12 * j + k];
        wc_load12(S, WC_A, v);
        if (var == 1) wc_copy(S, WC_B, WC_A);
      }
      if (threadIdx.x == 0) {
        wc_store(r, S, var == 0 ? WC_A : WC_B);
        const fp* pr = &r.c0.c0.c0;
        for (int j = 0; j < 12; j++)
          for (int k = 0; k < 12; k++) out[12 * j + k] = pr[j].l[k];
        out[144] = 0;
      }
      return;
    }
    case W_IS_ONE:
      slot_in(S, WC_A, a);
      res = WC_A;
      flag = wc_is_one(S, WC_A) ? 1u : 0u;
      break;
    case W_EXP_X:
      slot_in(S, WC_A, a);
      if (var == 1) res = WC_A;
      wc_exp_x(S, res, WC_A);
      break;
    case W_FINAL_EXP:
      slot_in(S, var == 1 ? WC_F : WC_C, a);
      res = WC_F;
      wc_final_exp(S, WC_F, var == 1 ? WC_F : WC_C);
      flag = wc_is_one(S, WC_F) ? 1u : 0u;
      break;
    default: return;
  }
  slot_out(out, S, res);
  if (threadIdx.x == 0) out[144] = flag;
}

// workgroup i: the Miller value of pair qs[i] from the stored lines of n_pairs pairs
LBT_KERNEL k_wc_miller(uint32_t n_pairs, const uint32_t* __restrict__ lines, uint32_t nq, const uint32_t* __restrict__ qs,
                       uint32_t* __restrict__ out) {
  __shared__ wc_smem S;
  const uint32_t i = blockIdx.x;
  if (i >= nq) return;
  const uint32_t q = qs[i];
  if (q >= n_pairs) return;
  wc_init_tables(S);
  wc_miller_from_lines(S, WC_FS, lines, n_pairs, q);
  slot_out(out + (size_t)144 * i, S, WC_FS);
}
}  // namespace

// Words per record (a, b, out) of op; b = 0: not read.  0 = ok, 1 = unknown op.
extern "C" int lbt_wc_op_widths(int op, uint32_t* w) {
  if (op < W_APPLY || op > W_FINAL_EXP) return 1;
  w[0] = 144;
  w[1] = op == W_APPLY ? 144 : 0;
  w[2] = 145;
  return 0;
}

// Host-buffer entry: n cases, one workgroup each.  0 = ok.
extern "C" int lbt_wc_op(int op, int wop, int var, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  uint32_t w[3];
  if (lbt_wc_op_widths(op, w) || n == 0 || !a || !out || (w[1] && !b) || wop < 0 || wop >= LB_WC_NOPS) return 5;
  uint32_t *da = nullptr, *db = nullptr, *dout = nullptr;
  if (hipMalloc(&da, (size_t)n * 144 * 4) != hipSuccess || hipMalloc(&db, (size_t)n * 144 * 4) != hipSuccess ||
      hipMalloc(&dout, (size_t)n * 145 * 4) != hipSuccess)
    return 1;
  int rc = 0;
  if (hipMemcpy(da, a, (size_t)n * 144 * 4, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
  if (!rc && (w[1] ? hipMemcpy(db, b, (size_t)n * 144 * 4, hipMemcpyHostToDevice)
                   : hipMemset(db, 0, (size_t)n * 144 * 4)) != hipSuccess)
    rc = 2;
  if (!rc && hipMemset(dout, 0, (size_t)n * 145 * 4) != hipSuccess) rc = 2;
  if (!rc) {
    hipLaunchKernelGGL(k_wc, dim3(n), dim3(TPB), 0, 0, op, wop, var, n, da, db, dout);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 3;
  }
  if (!rc && hipMemcpy(out, dout, (size_t)n * 145 * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = 4;
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  return rc;
}

// wc_miller_from_lines over a line array of n_pairs pairs (68 * 72 * n_pairs words) for the
// nq pairs listed in qs (each < n_pairs): out = nq x 144 words.  0 = ok.
extern "C" int lbt_wc_miller(uint32_t n_pairs, const uint32_t* lines, uint32_t nq, const uint32_t* qs, uint32_t* out) {
  if (n_pairs == 0 || nq == 0 || !lines || !qs || !out) return 5;
  for (uint32_t i = 0; i < nq; i++)
    if (qs[i] >= n_pairs) return 5;
  const size_t total = (size_t)LB_MILLER_LINES * 72 * n_pairs;
  uint32_t *dl = nullptr, *dq = nullptr, *dout = nullptr;
  if (hipMalloc(&dl, total * 4) != hipSuccess || hipMalloc(&dq, (size_t)nq * 4) != hipSuccess ||
      hipMalloc(&dout, (size_t)nq * 144 * 4) != hipSuccess)
    return 1;
  int rc = 0;
  if (hipMemcpy(dl, lines, total * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dq, qs, (size_t)nq * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dout, 0, (size_t)nq * 144 * 4) != hipSuccess)
    rc = 2;
  if (!rc) {
    hipLaunchKernelGGL(k_wc_miller, dim3(nq), dim3(TPB), 0, 0, n_pairs, dl, nq, dq, dout);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 3;
  }
  if (!rc && hipMemcpy(out, dout, (size_t)nq * 144 * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = 4;
  (void)hipFree(dl);
  (void)hipFree(dq);
  (void)hipFree(dout);
  return rc;
}
