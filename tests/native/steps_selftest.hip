// Test-only library for tests/test_gpu_line_pairs.py: the step-major accumulation of k_steps.hip
// over lines the test supplies, once by k_step_acc on the raw lines and once by k_line_pairs +
// k_step_acc<.., true>, with the row layout built by the product's own kernels.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "k_steps.hip"

using namespace lb;

#define ST_HIP(x)                 \
  do {                            \
    if ((x) != hipSuccess) {      \
      rc = __LINE__;              \
      goto done;                  \
    }                             \
  } while (0)

template <bool PRE>
static decltype(&k_step_acc<0, 1>) st_kernel(int mode) {
  return mode == 1 ? k_step_acc<1, 1, PRE> : k_step_acc<0, 1, PRE>;
}

extern "C" {

// One call of n_req requests (req_off: n_req + 1 offsets into the n_sets sets), its n_pairs =
// n_sets + n_req + 1 line slots given in `lines` (n_pairs x 68 x 72 words, the pipeline's SoA).
//   G_raw:   k_step_acc<mode, 1> on the lines as given          (144 x n_sets x split words)
//   G_pre:   k_line_pairs, then k_step_acc<mode, 1, true>
//   lines_after: the lines buffer after k_line_pairs
//   rowoff (n_sets + 1), pos (n_req): the row layout (set i of request k at slot rowoff[i] + pos[k])
// Returns 0, or the source line of the HIP call that failed.
int st_run(uint32_t n_req, const uint32_t* req_off, const uint32_t* lines, int mode, uint32_t split, uint32_t* G_raw,
           uint32_t* G_pre, uint32_t* lines_after, uint32_t* rowoff, uint32_t* pos) {
  int rc = 0;
  const uint32_t n_sets = req_off[n_req], n_pairs = n_sets + n_req + 1, ns = n_sets ? n_sets : 1;
  const size_t line_words = (size_t)n_pairs * LB_MILLER_LINES * 72, g_words = (size_t)144 * ns * split;
  if ((mode != 0 && mode != 1) || (split != 1 && split != 2 && split != 4) || !n_sets) return -1;
  uint32_t *d_off = nullptr, *d_lines = nullptr, *d_G = nullptr, *d_rows = nullptr;
  // rows: hist + cursors 2 (ns + 1), gt ns + 1, rowoff ns + 1, pos n_req, inv n_req, meta 1
  const size_t rows_words = 4 * ((size_t)ns + 1) + 2 * (size_t)n_req + 1;
  ST_HIP(hipMalloc(&d_off, ((size_t)n_req + 1) * 4));
  ST_HIP(hipMalloc(&d_lines, line_words * 4));
  ST_HIP(hipMalloc(&d_G, g_words * 4));
  ST_HIP(hipMalloc(&d_rows, rows_words * 4));
  {
    uint32_t *d_hist = d_rows, *d_cur = d_hist + (ns + 1), *d_gt = d_cur + (ns + 1), *d_rowoff = d_gt + (ns + 1);
    uint32_t *d_pos = d_rowoff + (ns + 1), *d_inv = d_pos + n_req, *d_meta = d_inv + n_req;
    ST_HIP(hipMemcpy(d_off, req_off, ((size_t)n_req + 1) * 4, hipMemcpyHostToDevice));
    ST_HIP(hipMemset(d_rows, 0, rows_words * 4));
    k_rows_hist<<<(n_req + 255) / 256, 256>>>(n_req, d_off, d_hist);
    k_rows_scan<<<1, 1024>>>(n_sets, d_hist, d_gt, d_rowoff, d_meta);
    k_rows_pos<<<(n_req + 255) / 256, 256>>>(n_req, d_off, d_gt, d_cur, d_pos, d_inv);
    ST_HIP(hipGetLastError());
    ST_HIP(hipDeviceSynchronize());
    const Rows R{d_rowoff, d_inv, d_pos, d_meta, split};
    const uint32_t lanes = n_sets * split, grid = (lanes + TPB - 1) / TPB;
    const uint32_t pair_threads = lanes * ((uint32_t)LB_MILLER_LINES / split / 2u);
    ST_HIP(hipMemcpy(d_lines, lines, line_words * 4, hipMemcpyHostToDevice));
    ST_HIP(hipMemset(d_G, 0, g_words * 4));
    st_kernel<false>(mode)<<<grid, TPB>>>(n_sets, n_pairs, R, d_off, d_lines, d_G);
    ST_HIP(hipGetLastError());
    ST_HIP(hipDeviceSynchronize());
    ST_HIP(hipMemcpy(G_raw, d_G, g_words * 4, hipMemcpyDeviceToHost));
    ST_HIP(hipMemset(d_G, 0, g_words * 4));
    k_line_pairs<<<(pair_threads + TPB - 1) / TPB, TPB>>>(n_sets, n_pairs, R, d_off, d_lines);
    ST_HIP(hipGetLastError());
    ST_HIP(hipDeviceSynchronize());
    ST_HIP(hipMemcpy(lines_after, d_lines, line_words * 4, hipMemcpyDeviceToHost));
    st_kernel<true>(mode)<<<grid, TPB>>>(n_sets, n_pairs, R, d_off, d_lines, d_G);
    ST_HIP(hipGetLastError());
    ST_HIP(hipDeviceSynchronize());
    ST_HIP(hipMemcpy(G_pre, d_G, g_words * 4, hipMemcpyDeviceToHost));
    ST_HIP(hipMemcpy(rowoff, d_rowoff, ((size_t)ns + 1) * 4, hipMemcpyDeviceToHost));
    ST_HIP(hipMemcpy(pos, d_pos, (size_t)n_req * 4, hipMemcpyDeviceToHost));
  }
done:
  hipFree(d_off);
  hipFree(d_lines);
  hipFree(d_G);
  hipFree(d_rows);
  return rc;
}

}  // extern "C"
