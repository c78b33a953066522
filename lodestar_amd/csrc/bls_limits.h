// The pipeline's numeric limits that host planning and the kernels share: plain C++, no HIP,
// so bls_plan.h builds with a host compiler.  bls_pairing.h, bls_kernels.h and bls_lp.h
// include this file; each limit is defined here and nowhere else.
#pragma once
#include <stdint.h>

// Bucket MSM of the merged check (k_msm.hip): signed digits of LB_MSM_C bits in
// LB_MSM_W windows of the 32-bit GLV half-scalars, LB_MSM_NB buckets per window,
// chunks of <= LB_MSM_T entries, bit positions 0 .. LB_MSM_POS - 1.
#define LB_MSM_C 11
#define LB_MSM_W 3
#define LB_MSM_NB 1024u
#define LB_MSM_BUCKETS (LB_MSM_W * LB_MSM_NB)
#define LB_MSM_T 16u
#define LB_MSM_T_LONE 4u  // (a lone call of at most LB_LP_DEC_MAX sets: shorter chunk chains, more chunks)
#define LB_MSM_POS 33u
#define LB_MSM_NONE 0xffffffffu

// Round programs (k_lp.hip): workgroup shapes, and the size bounds and record counts of the
// programs a pipeline call runs
#ifndef LB_LP_ROWS
#define LB_LP_ROWS 32                     // units per round = 16-lane rows per workgroup
#endif
#define LB_LP_TPB (LB_LP_ROWS * 16)       // 8 waves: 2 per SIMD (256 VGPRs for the one-lane inversion)
#define LB_LP_TREE_LEVELS 20              // product-tree levels (requests up to 2^20 sets)
#define LB_LP_NARROW_ROWS 8  // gen_lp.py DEC_ROWS
#define LB_LP_LINES_MAX 5120  // lone steps calls of at most this many sets store their lines via k_lp_lines (6,144: -0.5 ms)
#define LB_LP_LINES_NOUT (68 * 6)
#define LB_LP_HF_ROWS 16           // gen_lp.py HF_ROWS
#define LB_LP_HF_MAX 3072          // lone calls of at most this many sets finish their hash on k_lp_hf
#define LB_LP_DEC_ROWS 8          // gen_lp.py DEC_ROWS
#define LB_LP_DEC_MAX 5120        // ... and lone pipeline calls of at most this many sets
#define LB_MSM_BITS_GROUP 8      // lpgen/bls.py MSM_BITS_GROUP
#define LB_MSM_BITS_INST (LB_MSM_POS * (LB_MSM_NB / 2 / LB_MSM_BITS_GROUP))  // level-0 instances: 33 x 64
#define LB_RTAIL_NIN 16                 // rtail inputs: F_k (12 Fp), S_k affine (4 Fp); inflag S_inf
#define LB_MTAIL_LEVELS 63                  // the step-major accumulation's Horner levels (k_steps.hip)
#define LB_MTAIL_NIN (12 * LB_MTAIL_LEVELS + 6 * LB_MSM_POS)  // mtail inputs: the 63 level products, the MSM's
                                                              // 33 bit sums

// Steps calls of at least LB_PAIR_PRE_MIN_SETS sets whose lines k_lines_rows stores multiply their
// line pairs in k_line_pairs ahead of k_step_acc (k_steps.hip): above the LB_LP_LINES_MAX band of
// the round-program lines.  LB_PAIR_PRE=0 at compile time removes the rule (the A/B build).
#ifndef LB_PAIR_PRE
#define LB_PAIR_PRE 1
#endif
#define LB_PAIR_PRE_MIN_SETS 8192

namespace lb {
// the 68 lines of one pair (63 doubling + 5 addition steps, loop order): bls_pairing.h
static constexpr int LB_MILLER_LINES = 68;
static constexpr uint32_t LB_LP_NIN = 11, LB_LP_NFL = 67;  // the latency path's set program: inputs / input flags
static constexpr uint32_t LB_MSM_BLANES = 4;      // k_msm_buckets: lanes per bucket
static constexpr uint32_t LB_MSM_BITS_TPB = 256;  // k_msm_bits: threads per bit position
// the level products in two stages (round 6): lane products of each level's share, then
// wave-cooperative products of groups of LB_LVL_GROUP partials (k_steps.hip)
static constexpr uint32_t LB_LVL_GROUP = 8;
}  // namespace lb
