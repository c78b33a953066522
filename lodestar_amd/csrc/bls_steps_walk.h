// The walk of one lane of the step-major accumulation (k_steps.hip) over its lines, as integer
// arithmetic: plain C++17 that also compiles for the device, so k_step_acc, k_line_pairs and a
// host test (tests/native/steps_walk_host.cpp) enumerate a lane's items with the same code.
//
// A lane of an n-set request takes L consecutive lines t in [t0, t0 + L) of the request in
// step-major order, line t being (step j = t / n, pair i = t mod n).  Its items, in order: two
// lines (j, i), (j, i + 1) of one step at once -- a pair -- when both belong to the step
// (i + 1 < n) and to the lane (two lines remain), else one line; i wraps at n into the next
// step.  Every line of the request is in exactly one item of one lane.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LB_WALK_FN __host__ __device__ inline
#else
#define LB_WALK_FN inline
#endif

namespace lb {

struct StepItem {
  uint32_t j, i;  // the item's (first) line: step and pair index
  bool paired;    // with line (j, i + 1)
};

struct StepWalk {
  uint32_t n, j, i, left;
  bool pairs;  // false: one line at a time (k_step_acc MODE 2)
  LB_WALK_FN StepWalk(uint32_t n_, uint32_t t0, uint32_t L, bool pairs_)
      : n(n_), j(t0 / n_), i(t0 - (t0 / n_) * n_), left(L), pairs(pairs_) {}
  LB_WALK_FN bool done() const { return left == 0; }
  LB_WALK_FN StepItem next() {
    const StepItem it{j, i, pairs && i + 1 < n && left > 1};
    const uint32_t k = it.paired ? 2u : 1u;
    i += k;
    left -= k;
    if (i >= n) {
      i -= n;
      j++;
    }
    return it;
  }
};

// The u-th pair (u = 0, 1, ...) of the lane -> its (j, i); false when the lane has at most u pairs
// (at most L / 2 of them: a pair takes two of the lane's L lines)
LB_WALK_FN bool step_walk_pair(uint32_t n, uint32_t t0, uint32_t L, uint32_t u, uint32_t& j, uint32_t& i) {
  if (n < 2) return false;
  StepWalk w(n, t0, L, true);
  while (!w.done()) {
    const StepItem it = w.next();
    if (!it.paired) continue;
    if (u == 0) {
      j = it.j;
      i = it.i;
      return true;
    }
    u--;
  }
  return false;
}

}  // namespace lb
