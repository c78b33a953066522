// Test-only HIP library, one-lane half: the Miller steps, the stored-line Miller loop,
// miller_loop, final_exp and fp12_exp_x of bls_pairing.h, one case per lane.  (The
// wave-cooperative half is pairing_wc_selftest.hip; both link into
// libpairing_selftest.so.)  Values travel as raw little-endian 32-bit limbs in
// Montgomery form: an Fp2 is 24 words, a projective T is X | Y | Z (72 words), an
// Fp12 is its 12 coefficients in tower order (144 words), a line is l0 | l1 | l4
// (72 words).  tests/test_gpu_pairing.py converts and normalises in Python, so no
// routine under test sits in the I/O path.  Never linked into the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bls_kernels.h"

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
LB_DEV void ld_proj(g2proj& t, const uint32_t* w) {
  ldw(t.X, w);
  ldw(t.Y, w + 24);
  ldw(t.Z, w + 48);
}
LB_DEV void st_proj(uint32_t* w, const g2proj& t) {
  stw(w, t.X);
  stw(w + 24, t.Y);
  stw(w + 48, t.Z);
}

// the launch bound of the product's tail kernels
#define LBT_KERNEL __global__ void __launch_bounds__(TPB, LB_W_TAIL)

enum { P_DBL = 0, P_ADD, P_MILLER = 10, P_FINAL_EXP, P_EXP_X };
enum { L_LINES = 0, L_LINES_QMEM };

// a = T | xp | yp (96 words), b = xq | yq (48, P_ADD), out = T' | l0 | l1 | l4 (144).
// P_DBL var 1: miller_dbl_step_put through a one-pair buffer (the line half of the
// lane's own output record: n_pairs = 1, q = 0, j = 0).
LBT_KERNEL k_step(int op, int var, uint32_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                  uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a += (size_t)96 * i;
  out += (size_t)144 * i;
  g2proj T;
  fp xp, yp;
  ld_proj(T, a);
  ldw(xp, a + 72);
  ldw(yp, a + 84);
  fp2 l0, l1, l4;
  if (op == P_DBL && var == 1) {
    miller_dbl_step_put(T, xp, yp, out + 72, 1, 0, 0);
    st_proj(out, T);
    return;
  }
  if (op == P_DBL) {
    miller_dbl_step(T, l0, l1, l4, xp, yp);
  } else {
    fp2 xq, yq;
    ldw(xq, b + (size_t)48 * i);
    ldw(yq, b + (size_t)48 * i + 24);
    miller_add_step(T, xq, yq, l0, l1, l4, xp, yp);
  }
  st_proj(out, T);
  stw(out + 72, l0);
  stw(out + 96, l1);
  stw(out + 120, l4);
}

// pq = x | y | inf of P (25 words), x | y | inf of Q (49 words) per pair; lane q stores
// the 68 lines of pair q.  qj (L_LINES_QMEM): Q as a Jacobian record in memory.
LBT_KERNEL k_lines(int var, uint32_t n_pairs, const uint32_t* __restrict__ pq, g2j* __restrict__ qj,
                   uint32_t* __restrict__ lines) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_pairs) return;
  pq += (size_t)74 * q;
  g1a P;
  ldw(P.x, pq);
  ldw(P.y, pq + 12);
  P.inf = pq[24] != 0;
  g2a Q;
  ldw(Q.x, pq + 25);
  ldw(Q.y, pq + 49);
  Q.inf = pq[73] != 0;
  if (var == L_LINES) {
    miller_lines(P, Q, lines, n_pairs, q);
  } else {
    qj[q].X = Q.x;
    qj[q].Y = Q.y;
    fp2_one(qj[q].Z);
    miller_lines_qmem(P, &qj[q], lines, n_pairs, q);
  }
}

// out[(q * 68 + j) * 72 ...] = line j of pair q as line_get reads it
LBT_KERNEL k_line_get(uint32_t n_pairs, const uint32_t* __restrict__ lines, uint32_t* __restrict__ out) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_pairs) return;
#pragma unroll 1
  for (int j = 0; j < LB_MILLER_LINES; j++) {
    fp2 l0, l1, l4;
    line_get(lines, n_pairs, q, j, l0, l1, l4);
    uint32_t* o = out + ((size_t)q * LB_MILLER_LINES + j) * 72;
    stw(o, l0);
    stw(o + 24, l1);
    stw(o + 48, l4);
  }
}

// P_MILLER: a = xp | yp (24), b = xq | yq (48); P_FINAL_EXP, P_EXP_X: a = Fp12; out = Fp12
LBT_KERNEL k_lane12(int op, uint32_t n, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                    uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  fp12 f, r;
  if (op == P_MILLER) {
    g1a P;
    g2a Q;
    ldw(P.x, a + (size_t)24 * i);
    ldw(P.y, a + (size_t)24 * i + 12);
    ldw(Q.x, b + (size_t)48 * i);
    ldw(Q.y, b + (size_t)48 * i + 24);
    P.inf = Q.inf = false;
    miller_loop(r, P, Q);
  } else {
    ldw(f, a + (size_t)144 * i);
    if (op == P_FINAL_EXP)
      final_exp(r, f);
    else
      fp12_exp_x(r, f);
  }
  stw(out + (size_t)144 * i, r);
}

bool widths(int op, uint32_t w[3]) {
  switch (op) {
    case P_DBL: w[0] = 96; w[1] = 0; w[2] = 144; return true;
    case P_ADD: w[0] = 96; w[1] = 48; w[2] = 144; return true;
    case P_MILLER: w[0] = 24; w[1] = 48; w[2] = 144; return true;
    case P_FINAL_EXP: case P_EXP_X: w[0] = 144; w[1] = 0; w[2] = 144; return true;
    default: return false;
  }
}
}  // namespace

// Words per record (a, b, out) of op; 0 = ok, 1 = unknown op.
extern "C" int lbt_pairing_op_widths(int op, uint32_t* w) { return widths(op, w) ? 0 : 1; }

// Host-buffer entry: n records of a (and of b where the op takes one), n records out.  0 = ok.
extern "C" int lbt_pairing_op(int op, int var, uint32_t n, const uint32_t* a, const uint32_t* b, uint32_t* out) {
  uint32_t w[3];
  if (!widths(op, w) || n == 0 || !a || !out || (w[1] && !b)) return 5;
  uint32_t *da = nullptr, *db = nullptr, *dout = nullptr;
  if (hipMalloc(&da, (size_t)n * w[0] * 4) != hipSuccess || hipMalloc(&db, (size_t)n * (w[1] ? w[1] : 1) * 4) != hipSuccess ||
      hipMalloc(&dout, (size_t)n * w[2] * 4) != hipSuccess)
    return 1;
  int rc = 0;
  if (hipMemcpy(da, a, (size_t)n * w[0] * 4, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
  if (!rc && w[1] && hipMemcpy(db, b, (size_t)n * w[1] * 4, hipMemcpyHostToDevice) != hipSuccess) rc = 2;
  if (!rc && hipMemset(dout, 0, (size_t)n * w[2] * 4) != hipSuccess) rc = 2;
  if (!rc) {
    const dim3 grid((n + TPB - 1) / TPB), block(TPB);
    if (op < P_MILLER)
      hipLaunchKernelGGL(k_step, grid, block, 0, 0, op, var, n, da, db, dout);
    else
      hipLaunchKernelGGL(k_lane12, grid, block, 0, 0, op, n, da, db, dout);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 3;
  }
  if (!rc && hipMemcpy(out, dout, (size_t)n * w[2] * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = 4;
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  return rc;
}

// Words of one pair's record in pq, and of one pair's lines.
extern "C" int lbt_pairing_lines_widths(uint32_t* w) {
  w[0] = 74;
  w[1] = LB_MILLER_LINES * 72;
  return 0;
}

// The stored lines of n_pairs pairs (var 0: miller_lines, 1: miller_lines_qmem).  buf holds
// guard + 68 * 72 * n_pairs + guard words, pre-filled by the caller; the line array starts
// at buf + guard and the whole buffer comes back.  0 = ok.
extern "C" int lbt_pairing_lines(int var, uint32_t n_pairs, uint32_t guard, const uint32_t* pq, uint32_t* buf) {
  if ((var != L_LINES && var != L_LINES_QMEM) || n_pairs == 0 || !pq || !buf) return 5;
  const size_t total = (size_t)LB_MILLER_LINES * 72 * n_pairs + 2 * (size_t)guard;
  uint32_t *dpq = nullptr, *dbuf = nullptr;
  g2j* dq = nullptr;
  if (hipMalloc(&dpq, (size_t)n_pairs * 74 * 4) != hipSuccess || hipMalloc(&dbuf, total * 4) != hipSuccess ||
      hipMalloc(&dq, (size_t)n_pairs * sizeof(g2j)) != hipSuccess)
    return 1;
  int rc = 0;
  if (hipMemcpy(dpq, pq, (size_t)n_pairs * 74 * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dbuf, buf, total * 4, hipMemcpyHostToDevice) != hipSuccess)
    rc = 2;
  if (!rc) {
    hipLaunchKernelGGL(k_lines, dim3((n_pairs + TPB - 1) / TPB), dim3(TPB), 0, 0, var, n_pairs, dpq, dq, dbuf + guard);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 3;
  }
  if (!rc && hipMemcpy(buf, dbuf, total * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = 4;
  (void)hipFree(dpq);
  (void)hipFree(dbuf);
  (void)hipFree(dq);
  return rc;
}

// line_get over a line array of n_pairs pairs: out = n_pairs x 68 x 72 words.  0 = ok.
extern "C" int lbt_pairing_line_get(uint32_t n_pairs, const uint32_t* lines, uint32_t* out) {
  if (n_pairs == 0 || !lines || !out) return 5;
  const size_t total = (size_t)LB_MILLER_LINES * 72 * n_pairs;
  uint32_t *dl = nullptr, *dout = nullptr;
  if (hipMalloc(&dl, total * 4) != hipSuccess || hipMalloc(&dout, total * 4) != hipSuccess) return 1;
  int rc = 0;
  if (hipMemcpy(dl, lines, total * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemset(dout, 0, total * 4) != hipSuccess)
    rc = 2;
  if (!rc) {
    hipLaunchKernelGGL(k_line_get, dim3((n_pairs + TPB - 1) / TPB), dim3(TPB), 0, 0, n_pairs, dl, dout);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 3;
  }
  if (!rc && hipMemcpy(out, dout, total * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = 4;
  (void)hipFree(dl);
  (void)hipFree(dout);
  return rc;
}
