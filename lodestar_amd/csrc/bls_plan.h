// Planning of a throughput-pipeline call (bls_host.hip run_pipeline), as host arithmetic:
// plain C++17, no HIP, so the rules are testable without a GPU (tests/native/plan_host.cpp).
//
//   PipeConfig       the switches that shape a call (LB_* environment, config_from_env)
//   PipeShape        what is known of a call when it is submitted
//   plan_pipeline    every decision of the call: organisation, merged check, MSM, round
//                    programs, kernel variants
//   plan_upper       the plan whose layout bounds that of any call with at most that many
//                    requests and sets (pipeline_ws_bytes: sizing ahead of a call)
//   layout_pipeline  every workspace buffer of a plan: offsets and the total, in bytes
//                    (carved by bls_carve.h's rule, which also lays out what the callers put
//                    in front of the pipeline's workspace)
//
// run_pipeline builds plan and layout, checks the slab once, and enqueues; nothing below the
// plan reads a switch or compares a size.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bls_carve.h"
#include "bls_limits.h"

namespace lb {

// ---- the switches -----------------------------------------------------------------------
struct PipeConfig {
  // Miller organisation: stored lines + one wave per pair (k_lines/k_pair_wc,
  // lowest latency) up to wave_max_sets; one pair per lane (k_miller_sets)
  // below lines_min_sets; stored lines + multi-pair accumulation per request
  // (k_lines/k_miller_acc, highest throughput) from there.  LB_MILLER=wave|lane|lines forces one.
  int miller_mode = 0;  // 0 auto, 1 lane, 2 lines, 3 wave
  // 1025: every call the latency path does not take (lp_max_sets) uses the stored lines;
  // 1.5k-6k-set calls 25-29 -> 17-19 ms, C5 27.2 -> 21.0 ms (profiles/r06/orgs_probe_r06f.json)
  uint32_t lines_min_sets = 1025;
  uint32_t wave_max_sets = 1024;
  // LB_LINES_WAVES: 1 or 2 waves/SIMD for k_lines(_rows): 2 spills (3.4 -> 4.7 ms alone) but its
  // waves share SIMDs with other calls' in the pipeline (profiles/ab_r03/ab_r03r, ab_r03s)
  int lines_waves = 2;
  int lines_waves_small = 1;  // k_lines for the calls below the steps organisation
  int acc_lpr = 64;     // LB_ACC_LPR: lanes per request in k_miller_acc (64, 32, 16)
  int acc_split = -1;   // LB_ACC_SPLIT: 1 always / 0 never split requests in halves; -1 = lone calls only
  // Miller accumulation of the stored lines: 1 = step-major lanes + level products +
  // one Horner chain (k_steps.hip, default), 0 = pair-major k_miller_acc (LB_ACC=pairs)
  int acc_steps = 1;
  // LB_STEP_MODE: k_step_acc variant (0 registers + paired lines, 1 accumulator in LDS,
  // 2 registers + one line at a time; k_steps.hip)
  // defaults (round 4): the accumulator in LDS at one wave per SIMD -- alone 4.64-4.70 ms per
  // C2 launch against 6.04-6.10 for one line at a time at 2 waves/SIMD (which spilled 1,408
  // B/lane: 18.3 GB of traffic per launch, 13.9x the algorithmic bytes; now 2.6 GB, 2.0x), the
  // pipeline 3.55-3.62 vs 3.54-3.57 M sets/s, three interleaved runs each
  // (profiles/r04/step_ab/).  Round 3 had measured 2/2 ahead of 2/1 (profiles/ab_r03/ab_r03s).
  // Round 5, in the final pipeline (merged-check program, two-phase flow): one line at a time
  // at 2 waves/SIMD (LB_STEP_MODE=2 LB_STEP_WAVES=2) measured ahead -- 3.61-3.67 M (mean 3.650
  // over 5 runs) against the LDS build's 3.53-3.61 M (mean 3.569) -- but alone it takes 5.7 ms
  // against 4.4-4.5 and moves 18.4 GB per launch (13.9x its algorithmic bytes: spills) against
  // 2.6 GB (profiles/r05/knobs/, final/pmc_traffic_r05s3.json); the LDS build stays the default
  // until a 2-wave build without the spills exists (half the accumulator in LDS: 18 KB a
  // workgroup, 8 per CU)
  int step_mode = 1;
  int step_waves = 1;  // LB_STEP_WAVES: occupancy target of k_step_acc (1 or 2)
  // per-request tails: one wave per request (k_lines_S + k_tail, wave-cooperative
  // Fp12) or LB_TAIL=lane: one lane per request (k_miller_S + k_final)
  bool tail_wave = true;
  // merged check of the whole call first (one tail), per-request tails only
  // when it fails; used from merge_min_req requests up (LB_MERGE_MIN, 0 = off)
  uint32_t merge_min_req = 8;
  // merged calls of at least msm_min_sets sets take S_all from the bucket MSM
  // (k_msm.hip) instead of per-set ladders (LB_MSM_MIN, 0 = never)
  uint32_t msm_min_sets = 1025;  // (same probe: from 1025 sets the MSM beats the ladders)
  // merged steps calls: the level products as lane products + wave-cooperative passes
  // (k_level_part / k_level_wc) instead of k_level_prod's one-lane LDS tree (LB_LEVEL=0)
  bool level_wc = true;
  // lone calls: the MSM's bucket sums on LB_MSM_BLANES lanes per bucket and its bit sums on 256
  // threads (LB_MSM_LANES=0: one lane per bucket and one wave per bit, round 5, always), the
  // merged-check program on 64 rows (LB_WIDE_TAIL=0: 32 rows always)
  bool msm_lanes = true;
  bool wide_tail = true;
  bool msm_bits_lp = true;  // (LB_MSM_BITS_LP=0: a lone call's bit sums by k_msm_bits' 256 threads)
  uint32_t step_split = 0;  // LB_STEP_SPLIT: 1, 2 or 4 lanes per set always (0: by size, lone calls only)
  // lone pipeline calls of at most LB_LP_DEC_MAX sets decode their signatures as round programs,
  // like small same-message packages (k_lp_dec; LB_LP_DECODE=0: k_decode_sigs)
  bool lp_decode = true;
  bool lp_hash_finish = true;  // (LB_LP_HASH_FINISH: the same calls' hash finish as round programs)
  bool msm_short = true;  // (LB_MSM_SHORT: a lone mid-size call's MSM chunks of LB_MSM_T_LONE entries)
  uint32_t msm_short_max = 16384u, msm_t_lone = LB_MSM_T_LONE;  // (LB_MSM_SHORT_MAX / LB_MSM_T_LONE probes)
  // (the lone-call round-program size bounds; env LB_LP_DEC_MAX / LB_LP_HF_MAX / LB_LP_LINES_MAX probe others)
  uint32_t lp_dec_max = LB_LP_DEC_MAX, lp_hf_max = LB_LP_HF_MAX, lp_lines_max = LB_LP_LINES_MAX;
  // (LB_LP_HASH_FULL: lone calls of at most this many sets run hash_to_G2's whole curve part as one
  // program per set, k_lp_hash -- profiles/r06/orgs_probe_r06hf3.json; 0: never)
  uint32_t lp_hash_full = 2048;
  uint32_t lp_narrow = 1;  // (LB_LP_NARROW=1: the hash-finish program on LB_LP_NARROW_ROWS rows, default; 0: 16 rows)
  bool lp_lines = true;  // (LB_LP_LINES: a lone steps call's lines as round programs, up to LB_LP_LINES_MAX sets)
  // latency path: calls of at most lp_max_sets sets run it instead of the throughput pipeline
  // (LB_LP_MAX, lb_set_latency_path; 0 = never)
  uint32_t lp_max_sets = 1024;
  uint32_t lp_lone_max = 896;  // (LB_LP_LONE_MAX, 0 = off: lone calls above it take the pipeline, plan_pipeline)
  bool lp_explicit = false;    // (the bound set by lb_set_latency_path / LB_LP_MAX: no lone rule)
  // the merged check of a steps + MSM call as a round program (k_lp_mtail: S_all from the
  // MSM's bit sums, Miller(-g1, S_all), final exponentiation on one workgroup) instead of
  // msm_final + lines of S_all + the one-wave k_tail (LB_MTAIL=0: the one-wave chain)
  bool mtail_lp = true;
  // LB_RTAIL (default 1): a failed merged check's per-request tails (Miller(-g1, S_k), F_k times
  // it, final exponentiation) as one round program per request (k_lp_rtail) instead of one-lane
  // lines of S_k (k_lines_S) + the one-wave chain (k_tail)
  bool rtail_lp = true;
  // LB_TP_RELEASE (default 1): a two-phase call completes as if the combined check passed and
  // frees its slot when its partial is out, instead of holding the slot through the host's
  // combine (-5..-7 % at N = 1); a failed combined check re-runs the shard
  // as a one-phase call.
  bool tp_release = true;  // the mode of the two-phase call being submitted
  // LB_TP_RELEASE as configured; after a failed combined check the next tp_pause_calls two-phase
  // calls take the legacy mode: a re-run repeats the whole shard (one wrong set per C2 call:
  // 1.07 M sets/s released against 1.98 M legacy, bench.py adversarial_two_phase), the legacy
  // mode runs only the per-request tails, so a stream of failing batches (invalid gossip)
  // costs the tails alone while a clean stream keeps the release
  bool tp_release_cfg = true;
};

// How an environment value becomes a field (every quirk of the switches is a kind of its own)
enum EnvKind : uint8_t {
  ENV_FLAG,      // atoi(v) != 0
  ENV_U32_ATOI,  // (uint32_t)atoi(v)
  ENV_U32,       // strtoul(v, 10)
  ENV_INT,       // atoi(v)
  ENV_MILLER,    // "lane" 1, "lines" 2, "wave" 3, anything else 0 (auto)
  ENV_NOT_LANE,  // LB_TAIL: false only for "lane"
  ENV_NOT_PAIRS,  // LB_ACC: 0 only for "pairs", else 1
  ENV_ONE_ELSE_2,  // LB_LINES_WAVES: 1 only for "1", else 2 -- both line kernels
  ENV_TWO_ELSE_1,  // LB_STEP_WAVES: 2 only for "2", else 1
  ENV_NONZERO_01,  // LB_ACC_SPLIT: 1 / 0 (never -1 again)
  ENV_LPR,         // LB_ACC_LPR: 64, 32 or 16, anything else ignored
  ENV_MSM_T_LONE,  // 1 .. LB_MSM_T, anything else ignored
  ENV_STEP_SPLIT,  // 1, 2 or 4, anything else 0 (by size)
  ENV_LP_MAX,      // clamped to [0, 2^LB_LP_TREE_LEVELS]; also sets lp_explicit
  ENV_TP_RELEASE,  // a flag into tp_release and tp_release_cfg
};
struct EnvKnob {
  const char* name;
  EnvKind kind;
  bool PipeConfig::*b;
  int PipeConfig::*i;
  uint32_t PipeConfig::*u;
};
inline constexpr EnvKnob env_b(const char* n, EnvKind k, bool PipeConfig::*f) { return {n, k, f, nullptr, nullptr}; }
inline constexpr EnvKnob env_i(const char* n, EnvKind k, int PipeConfig::*f) { return {n, k, nullptr, f, nullptr}; }
inline constexpr EnvKnob env_u(const char* n, EnvKind k, uint32_t PipeConfig::*f) { return {n, k, nullptr, nullptr, f}; }

static constexpr EnvKnob kEnvKnobs[] = {
    env_i("LB_MILLER", ENV_MILLER, &PipeConfig::miller_mode),
    env_b("LB_TAIL", ENV_NOT_LANE, &PipeConfig::tail_wave),
    env_u("LB_MERGE_MIN", ENV_U32_ATOI, &PipeConfig::merge_min_req),
    env_u("LB_MSM_MIN", ENV_U32_ATOI, &PipeConfig::msm_min_sets),
    env_u("LB_LINES_MIN", ENV_U32_ATOI, &PipeConfig::lines_min_sets),
    env_b("LB_LEVEL", ENV_FLAG, &PipeConfig::level_wc),
    env_b("LB_MSM_LANES", ENV_FLAG, &PipeConfig::msm_lanes),
    env_b("LB_WIDE_TAIL", ENV_FLAG, &PipeConfig::wide_tail),
    env_b("LB_MSM_BITS_LP", ENV_FLAG, &PipeConfig::msm_bits_lp),
    env_b("LB_LP_DECODE", ENV_FLAG, &PipeConfig::lp_decode),
    env_b("LB_LP_HASH_FINISH", ENV_FLAG, &PipeConfig::lp_hash_finish),
    env_b("LB_LP_LINES", ENV_FLAG, &PipeConfig::lp_lines),
    env_b("LB_MSM_SHORT", ENV_FLAG, &PipeConfig::msm_short),
    env_u("LB_LP_HASH_FULL", ENV_U32, &PipeConfig::lp_hash_full),
    env_u("LB_LP_NARROW", ENV_U32, &PipeConfig::lp_narrow),
    env_u("LB_LP_DEC_MAX", ENV_U32, &PipeConfig::lp_dec_max),
    env_u("LB_LP_HF_MAX", ENV_U32, &PipeConfig::lp_hf_max),
    env_u("LB_LP_LINES_MAX", ENV_U32, &PipeConfig::lp_lines_max),
    env_u("LB_MSM_SHORT_MAX", ENV_U32, &PipeConfig::msm_short_max),
    env_u("LB_MSM_T_LONE", ENV_MSM_T_LONE, &PipeConfig::msm_t_lone),
    env_u("LB_STEP_SPLIT", ENV_STEP_SPLIT, &PipeConfig::step_split),
    env_u("LB_WAVE_MAX", ENV_U32_ATOI, &PipeConfig::wave_max_sets),
    env_b("LB_MTAIL", ENV_FLAG, &PipeConfig::mtail_lp),
    env_b("LB_RTAIL", ENV_FLAG, &PipeConfig::rtail_lp),
    env_b("LB_TP_RELEASE", ENV_TP_RELEASE, &PipeConfig::tp_release),
    env_u("LB_LP_MAX", ENV_LP_MAX, &PipeConfig::lp_max_sets),
    env_u("LB_LP_LONE_MAX", ENV_U32, &PipeConfig::lp_lone_max),
    env_i("LB_LINES_WAVES", ENV_ONE_ELSE_2, &PipeConfig::lines_waves),
    env_i("LB_ACC_SPLIT", ENV_NONZERO_01, &PipeConfig::acc_split),
    env_i("LB_ACC", ENV_NOT_PAIRS, &PipeConfig::acc_steps),
    env_i("LB_STEP_MODE", ENV_INT, &PipeConfig::step_mode),
    env_i("LB_STEP_WAVES", ENV_TWO_ELSE_1, &PipeConfig::step_waves),
    env_i("LB_ACC_LPR", ENV_LPR, &PipeConfig::acc_lpr),
};

// Apply the environment (`lookup`: getenv, or a test's table) to the defaults in `c`.
inline void config_from_env(PipeConfig& c, const char* (*lookup)(const char*)) {
  for (const EnvKnob& k : kEnvKnobs) {
    const char* v = lookup(k.name);
    if (!v) continue;
    switch (k.kind) {
      case ENV_FLAG: c.*k.b = atoi(v) != 0; break;
      case ENV_U32_ATOI: c.*k.u = (uint32_t)atoi(v); break;
      case ENV_U32: c.*k.u = (uint32_t)strtoul(v, nullptr, 10); break;
      case ENV_INT: c.*k.i = atoi(v); break;
      case ENV_MILLER:
        c.*k.i = strcmp(v, "lane") == 0 ? 1 : strcmp(v, "lines") == 0 ? 2 : strcmp(v, "wave") == 0 ? 3 : 0;
        break;
      case ENV_NOT_LANE: c.*k.b = strcmp(v, "lane") != 0; break;
      case ENV_NOT_PAIRS: c.*k.i = strcmp(v, "pairs") ? 1 : 0; break;
      case ENV_ONE_ELSE_2: c.lines_waves = c.lines_waves_small = atoi(v) == 1 ? 1 : 2; break;
      case ENV_TWO_ELSE_1: c.*k.i = atoi(v) == 2 ? 2 : 1; break;
      case ENV_NONZERO_01: c.*k.i = atoi(v) ? 1 : 0; break;
      case ENV_LPR: {
        const int x = atoi(v);
        if (x == 64 || x == 32 || x == 16) c.*k.i = x;
        break;
      }
      case ENV_MSM_T_LONE: {
        const unsigned long t = strtoul(v, nullptr, 10);
        if (t >= 1 && t <= LB_MSM_T) c.*k.u = (uint32_t)t;
        break;
      }
      case ENV_STEP_SPLIT: {
        const int x = atoi(v);
        c.*k.u = (x == 1 || x == 2 || x == 4) ? (uint32_t)x : 0u;
        break;
      }
      case ENV_LP_MAX: {
        const long x = atol(v);  // clamped like lb_set_latency_path: the product tree's 2^LB_LP_TREE_LEVELS sets
        c.*k.u = x <= 0 ? 0u : x < (1l << LB_LP_TREE_LEVELS) ? (uint32_t)x : (1u << LB_LP_TREE_LEVELS);
        c.lp_explicit = true;
        break;
      }
      case ENV_TP_RELEASE: c.tp_release = c.tp_release_cfg = atoi(v) != 0; break;
    }
  }
}

// ---- the plan ---------------------------------------------------------------------------
struct PipeShape {
  uint32_t n_req = 0, n_sets = 0;
  bool lone = false;       // no other slot busy: the GPU is this call's
  bool partial = false;    // a two-phase call: stops at the merged product
  bool presigned = false;  // signatures already decoded and validated (same-message phase 2)
  bool prio_slot = false;  // submitted on the priority lane
};

// lone calls of lp_lone_max < n_sets <= lp_max_sets leave the latency path for the pipeline
// (plan_pipeline's lone_mid; the synchronous entry points then take slot 0's two-stream DAG)
inline bool lp_lone_rule(const PipeConfig& c, uint32_t n_sets) {
  return !c.lp_explicit && c.lp_lone_max && n_sets > c.lp_lone_max && n_sets <= c.lp_max_sets;
}

// lanes per set of a lone call's step-major accumulation: 4 up to 16,384 sets, 2 up to 32,768 (the
// call's lanes then fill at most one wave per SIMD), 1 above (profiles/r06/level_probe_r06x.json:
// 4,096 ... 16,384 sets 16.7-17.4 ms unsplit, 14.1-15.0 split in 4)
inline uint32_t step_split_for(uint32_t n_sets) { return n_sets <= 16384u ? 4u : n_sets <= 32768u ? 2u : 1u; }

// k_level_part's workgroups per level: one request per thread (a merged call's requests are
// mostly small), and about two lanes per thread when one large request holds the call
inline uint32_t level_blocks(uint64_t n_lanes, uint32_t n_req, bool wide) {
  // (wide, a lone call: about one lane per thread -- the products all in the wave-cooperative
  // passes, the fastest for the call; otherwise about two, one lane product each: less work)
  const uint64_t w = wide ? (4 * (uint64_t)n_req > n_lanes / 32u ? 4 * (uint64_t)n_req : n_lanes / 32u)
                          : (n_req > n_lanes / 126u ? n_req : n_lanes / 126u);
  const uint64_t b = (w + 255u) / 256u;
  return b < 1u ? 1u : b > 8u ? 8u : (uint32_t)b;
}

enum LinesKind : uint8_t { LINES_NONE, LINES_PLAIN, LINES_ROWS, LINES_LP };  // k_lines / k_lines_rows / k_lp_lines
enum DecodeKind : uint8_t { DECODE_NONE, DECODE_PLAIN, DECODE_LP };          // presigned / k_decode_sigs / k_lp_dec
enum HashKind : uint8_t { HASH_NONE, HASH_PLAIN, HASH_FINISH_LP, HASH_FULL_LP };

struct PipePlan {
  uint32_t n_req = 0, n_sets = 0;
  uint32_t ns = 1, nr1 = 1;  // buffer counts: at least one set, one request
  bool lone = false, partial = false, presigned = false;
  // calls of at most lp_max_sets sets run the latency path (run_lp) -- nothing below applies --
  // unless they are lone calls under the lone rule (lone_mid), which the pipeline runs as
  // steps + MSM + merged-check program: ~7.0 ms flat from ~400 sets against the latency
  // path's 7.2 / 8.0 ms at 896 / 1,024 sets (profiles/r06/orgs_probe_r06lp2.json), merged
  // whatever its request count; not when the latency-path bound was set explicitly
  bool latency_path = false, lone_mid = false;
  // organisation of the per-set Miller loops
  bool by_lines = false, by_wave = false;
  bool f_sets = false;     // per-set Miller values are kept (lane / wave organisations)
  bool lines_buf = false;  // the lines store: set pairs [0, n_sets), S pairs [n_sets, n_sets + n_req), the merged pair
  bool tail_wave = true;   // (a two-phase call always merges and uses the wave tails)
  bool merged = false;
  uint32_t n_pairs = 0;  // n_sets + n_req (+ the merged pair (-g1, S_all))
  bool use_msm = false;
  // stored lines accumulated step-major (k_steps.hip) or pair-major (k_miller_acc), where a lone
  // call splits every request in two halves: twice the waves at the price of the halves' separate
  // Fp12 squarings; with other calls in flight the idle SIMDs run their stages instead
  bool steps = false, split = false;
  // merged pair (-g1, S_all) with S_all from the MSM: without a split its Miller value is one extra
  // workgroup of k_miller_acc (fold), otherwise its lines are stored right after the MSM (lines_all)
  bool fold = false;
  // merged check as a round program (k_lp_mtail): S_all, its Miller value and the final
  // exponentiation from the MSM's bit sums and the 63 level products (their Horner chain folded in)
  bool mtail = false;
  // a lone call's serial tail in its wide forms (the GPU otherwise idle: latency is what counts):
  // the merged-check program on LB_LP_MTAIL_ROWS rows, the MSM's sums over more lanes.  With other
  // calls in flight the narrow forms, whose smaller workgroups wait for less of a CU (C2 3.62 vs
  // 3.67 / 3.68 M sets/s with either wide form in every call, profiles/r06/ab_r06k/)
  bool mt_wide = false, msm_wide = false;
  bool bits_lp = false;  // (and its bit sums as round programs: 9 dependent one-lane additions -> 3 launches)
  bool rtail = false;    // a merged call's failure path as round programs (k_lp_rtail)
  // bucket MSM: 2 half-points x W windows per set; a lone mid-size call takes chunks of
  // msm_t_lone entries (k_msm_chunks' chains are one lane's mixed additions, 16 of them ~2.5 ms for C5)
  size_t n_ent = 0, max_chunks = 0;
  bool msm_short = false;
  uint32_t msm_T = LB_MSM_T;
  // a lone mid-size call splits every lane of the step-major accumulation (its time is the
  // one-lane latency of a lane's 68 lines: 17 or 34 lines a lane instead; LB_STEP_SPLIT forces)
  uint32_t lsplit = 1;
  // a lone mid-size call's stages as round programs: signature decode up to lp_dec_max sets, hash
  // finish up to lp_hf_max (above that the workgroups queue: 1,536 / 2,048 sets 13.4 -> 11.0 /
  // 11.8 ms, 4,704 (C5) 16.1 -> 17.4, profiles/r06/orgs_probe_r06hf.json) or the whole curve part
  // of the hash up to lp_hash_full, the lines of a steps call up to lp_lines_max.
  // *_sets: the sets their records are sized for (0: no records)
  bool dec_lp = false, hf_lp = false, hash_full = false, hf_narrow = true, lines_lp = false;
  uint32_t dec_sets = 0, hf_sets = 0, ll_sets = 0;
  // the level products' two stages (k_level_part's partials, the first k_level_wc pass's output)
  bool level_wc = false;
  uint32_t lvl_per = 0;
  bool needs_lp = false;  // some stage runs a round program: they must be resident (lp_ensure)
  bool tp_release = true;
  // buffers only plan_upper asks for together with the others
  bool mt_out = false, fx = false, halves = false;
  // stages and kernel variants
  HashKind hash = HASH_NONE;
  LinesKind lines = LINES_NONE;
  DecodeKind decode = DECODE_NONE;
  bool miller_wave = false, miller_sets = false;
  int lines_W = 1;              // k_lines<W> / k_lines_rows<W>
  int step_M = 1, step_W = 1;   // k_step_acc<M, W>
  // the products of a lane's line pairs (line_mul_line: 6 of the 23 Fp2 products of a pair, which
  // touch no accumulator) in k_line_pairs, a two-wave kernel that shares SIMDs with other calls'
  // waves, ahead of the one-wave k_step_acc<M, W, true>; lone and shared calls alike
  bool pair_pre = false;
  int acc_lpr = 64;             // k_miller_acc<L>
};

inline PipePlan plan_pipeline(const PipeConfig& c, const PipeShape& s) {
  PipePlan p;
  const uint32_t n_sets = s.n_sets, n_req = s.n_req;
  p.n_req = n_req;
  p.n_sets = n_sets;
  p.ns = n_sets ? n_sets : 1;
  p.nr1 = n_req ? n_req : 1;
  p.lone = s.lone;
  p.partial = s.partial;
  p.presigned = s.presigned;
  p.lone_mid = !s.partial && !s.presigned && s.lone && !s.prio_slot && lp_lone_rule(c, n_sets) &&
               c.miller_mode == 0 && c.tail_wave && c.acc_steps;
  p.latency_path = !s.partial && !s.presigned && n_sets <= c.lp_max_sets && !p.lone_mid;
  p.by_lines = c.miller_mode == 2 || (c.miller_mode == 0 && n_sets >= c.lines_min_sets) || p.lone_mid;
  p.by_wave = !p.by_lines && (c.miller_mode == 3 || (c.miller_mode == 0 && n_sets <= c.wave_max_sets));
  p.f_sets = !p.by_lines;
  p.tail_wave = c.tail_wave || s.partial;
  p.lines_buf = p.by_lines || p.by_wave || p.tail_wave;
  p.merged = s.partial || (p.tail_wave && c.merge_min_req && n_req >= c.merge_min_req) || p.lone_mid;
  p.n_pairs = n_sets + n_req + (p.merged ? 1u : 0u);
  p.use_msm = p.merged && n_sets && c.msm_min_sets && (n_sets >= c.msm_min_sets || p.lone_mid);
  // steps organisation: no split (a request already has one lane per set)
  p.steps = p.by_lines && p.tail_wave && n_sets && c.acc_steps;
  p.split = p.by_lines && !p.steps && (c.acc_split == 1 || (c.acc_split < 0 && s.lone && n_req >= 64));
  p.halves = p.split;
  p.fold = p.use_msm && p.by_lines && !p.split && !p.steps;
  p.fx = p.fold;
  p.mtail = p.steps && p.use_msm && p.merged && c.mtail_lp;
  p.mt_out = p.mtail && s.partial;
  p.mt_wide = s.lone && c.wide_tail;
  p.msm_wide = s.lone && c.msm_lanes;
  p.bits_lp = p.msm_wide && p.mtail && c.msm_bits_lp;
  p.rtail = p.merged && p.tail_wave && c.rtail_lp;
  p.n_ent = p.use_msm ? 2 * (size_t)n_sets * LB_MSM_W : 0;
  p.msm_short = p.use_msm && s.lone && n_sets <= c.msm_short_max && c.msm_short;
  p.msm_T = p.msm_short ? c.msm_t_lone : LB_MSM_T;
  p.max_chunks = p.use_msm ? p.n_ent / p.msm_T + LB_MSM_BUCKETS : 0;
  if (p.steps) p.lsplit = c.step_split ? c.step_split : s.lone ? step_split_for(n_sets) : 1u;
  p.dec_lp = s.lone && !s.presigned && n_sets && n_sets <= c.lp_dec_max && c.lp_decode;
  p.hf_lp = s.lone && n_sets && n_sets <= c.lp_hf_max && c.lp_hash_finish;
  p.hash_full = p.hf_lp && n_sets <= c.lp_hash_full;
  p.hf_narrow = c.lp_narrow & 1u;
  p.lines_lp = p.steps && s.lone && n_sets <= c.lp_lines_max && c.lp_lines;
  p.dec_sets = p.dec_lp ? p.ns : 0;
  p.hf_sets = p.hf_lp ? p.ns : 0;
  p.ll_sets = p.lines_lp ? p.ns : 0;
  p.level_wc = p.steps && p.merged && c.level_wc;
  p.lvl_per = p.level_wc ? level_blocks((uint64_t)n_sets * p.lsplit, n_req, s.lone) * 256u : 0u;
  p.needs_lp = p.mtail || p.rtail || p.dec_lp || p.hf_lp || p.lines_lp;
  p.tp_release = c.tp_release;
  p.hash = !n_sets ? HASH_NONE : p.hash_full ? HASH_FULL_LP : p.hf_lp ? HASH_FINISH_LP : HASH_PLAIN;
  // (small calls are latency-bound: the spill-free one-wave k_lines unless LB_LINES_WAVES=2)
  p.lines = p.steps ? (p.lines_lp ? LINES_LP : LINES_ROWS)
                    : (n_sets && (p.by_lines || p.by_wave)) ? LINES_PLAIN : LINES_NONE;
  p.lines_W = (p.steps ? c.lines_waves : c.lines_waves_small) == 1 ? 1 : 2;
  p.miller_wave = n_sets && p.by_wave;
  p.miller_sets = n_sets && !p.by_wave && !p.by_lines;
  p.decode = (!n_sets || s.presigned) ? DECODE_NONE : p.dec_lp ? DECODE_LP : DECODE_PLAIN;
  p.step_M = c.step_mode == 1 ? 1 : c.step_mode == 2 ? 2 : 0;
  p.step_W = c.step_mode == 1 ? 1 : c.step_waves == 2 ? 2 : 1;
  p.pair_pre = LB_PAIR_PRE && p.steps && p.step_M != 2 && p.lines == LINES_ROWS && n_sets >= LB_PAIR_PRE_MIN_SETS;
  p.acc_lpr = c.acc_lpr == 16 ? 16 : c.acc_lpr == 32 ? 32 : 64;
  return p;
}

// The plan whose layout bounds the layout of every call of at most n_req requests and n_sets
// sets under this config, whatever its lone / partial / presigned state (which a caller that
// sizes a slab ahead of the call does not know): every optional buffer present, each at its
// largest -- 4 lanes per set or the forced split, the shorter of the two chunk lengths, the wide
// level partials, the round-program records for as many sets as a call that runs them can have.
inline PipePlan plan_upper(const PipeConfig& c, uint32_t n_req, uint32_t n_sets) {
  PipePlan p;
  p.n_req = n_req;
  p.n_sets = n_sets;
  p.ns = n_sets ? n_sets : 1;
  p.nr1 = n_req ? n_req : 1;
  p.lone = p.partial = true;
  p.f_sets = p.lines_buf = p.merged = p.use_msm = p.steps = p.split = p.halves = p.fold = p.fx = true;
  p.mtail = p.mt_out = p.bits_lp = p.rtail = p.level_wc = true;
  p.n_pairs = n_sets + n_req + 1u;
  p.n_ent = 2 * (size_t)n_sets * LB_MSM_W;
  p.msm_T = c.msm_t_lone < LB_MSM_T ? c.msm_t_lone : LB_MSM_T;
  p.max_chunks = p.n_ent / p.msm_T + LB_MSM_BUCKETS;
  p.lsplit = c.step_split ? c.step_split : 4u;
  p.lvl_per = level_blocks((uint64_t)n_sets * p.lsplit, n_req, true) * 256u;
  const auto capped = [&](bool on, uint32_t max_sets) { return !on || !max_sets ? 0u : p.ns < max_sets ? p.ns : max_sets; };
  p.dec_sets = capped(c.lp_decode, c.lp_dec_max);
  p.hf_sets = capped(c.lp_hash_finish, c.lp_hf_max);
  p.ll_sets = capped(c.lp_lines, c.lp_lines_max);
  return p;
}

// ---- the layout -------------------------------------------------------------------------
// One entry per workspace buffer of run_pipeline, in the order they are laid out
enum PipeBuf : int {
  PB_SIG, PB_RSIG, PB_Q, PB_H, PB_PK, PB_RPK, PB_F_SETS, PB_LINES, PB_SINGLE, PB_PK_ST, PB_SIG_ST,
  PB_S, PB_FS, PB_F, PB_RT_IN, PB_RT_FL, PB_BAD, PB_SALL, PB_FALL, PB_MFLAG, PB_MSTATS,
  PB_MKEYS, PB_MSORTED, PB_MHIST, PB_MCSUM, PB_MBSUM, PB_MG,
  PB_RHIST, PB_RGT, PB_ROWOFF, PB_RPOS, PB_RINV, PB_RMETA, PB_G, PB_FPARTS,
  PB_DEC_IN, PB_DEC_FL, PB_DEC_OUT, PB_DEC_OFL, PB_DEC_PRE, PB_HF_IN, PB_HF_OUT, PB_LL_IN, PB_LL_OUT,
  PB_PL, PB_LVA, PB_LVB, PB_LHA, PB_LHB, PB_MT_IN, PB_MT_OUT, PB_MB_IN0, PB_MB_IN1, PB_MB_IN2,
  PB_FX, PB_OFF2, PB_ACC_F, PB_ACC_BAD, PB_ACC_ERR, PB_PARTIAL,
  PB_COUNT
};
static constexpr const char* kPipeBufNames[PB_COUNT] = {
    "sig", "rsig", "q", "h", "pk", "rpk", "f_sets", "lines", "single", "pk_st", "sig_st",
    "S", "fS", "F", "rt_in", "rt_fl", "bad", "Sall", "Fall", "mflag", "mstats",
    "mkeys", "msorted", "mhist", "mcsum", "mbsum", "mG",
    "rhist", "rgt", "rowoff", "rpos", "rinv", "rmeta", "G", "Fparts",
    "dec_in", "dec_fl", "dec_out", "dec_ofl", "dec_pre", "hf_in", "hf_out", "ll_in", "ll_out",
    "Pl", "lvA", "lvB", "lhA", "lhB", "mt_in", "mt_out", "mb_in0", "mb_in1", "mb_in2",
    "Fx", "off2", "acc_F", "acc_bad", "acc_err", "partial"};

struct PipeLayout {
  static constexpr size_t kAbsent = kCarveAbsent;
  size_t off[PB_COUNT];    // offset from the slab's base, 256-aligned (kAbsent: the plan has no such buffer)
  size_t size[PB_COUNT];   // bytes
  size_t bytes = 0;        // end of the last buffer - start
  bool has(PipeBuf b) const { return off[b] != kAbsent; }
};

// Every buffer of a plan, laid out from `start` (the slab's fill when the call arrives) by
// carve_take: each aligned to 256 B, in one fixed order, so a plan that asks for more or
// larger buffers never ends before one that asks for fewer or smaller.
inline PipeLayout layout_pipeline(const PipePlan& p, size_t start = 0) {
  PipeLayout L;
  size_t at = start;
  const auto take = [&](PipeBuf b, bool present, size_t count, size_t elem) {
    L.off[b] = carve_take(at, count * elem, present);
    L.size[b] = present ? count * elem : 0;
  };
  if (p.latency_path) {  // run_lp's list (layout_lp) is the whole of it
    for (int b = 0; b < PB_COUNT; b++) take((PipeBuf)b, false, 0, 0);
    L.bytes = layout_lp(p.ns, true, start).end - start;
    return L;
  }
  const size_t ns = p.ns, nr = p.n_req, nr1 = p.nr1;
  take(PB_SIG, !p.presigned, ns, SZ_G2J);
  take(PB_RSIG, true, ns, SZ_G2J);
  take(PB_Q, true, 2 * ns, SZ_G2J);
  take(PB_H, true, ns, SZ_G2J);
  take(PB_PK, true, ns, SZ_G1J);
  take(PB_RPK, true, ns, SZ_G1J);
  take(PB_F_SETS, p.f_sets, ns, SZ_FP12);
  take(PB_LINES, p.lines_buf, (size_t)p.n_pairs * LB_MILLER_LINES * 72, 4);
  take(PB_SINGLE, true, ns, 1);
  take(PB_PK_ST, true, ns, 1);
  take(PB_SIG_ST, true, ns, 1);  // (unused when the caller passes the sets' status buffer or decoded signatures)
  take(PB_S, true, nr, SZ_G2A);
  take(PB_FS, true, nr, SZ_FP12);
  take(PB_F, true, nr, SZ_FP12);
  take(PB_RT_IN, p.rtail, nr1 * LB_RTAIL_NIN * 16, 4);
  take(PB_RT_FL, p.rtail, nr1, 4);
  take(PB_BAD, true, nr, 1);
  take(PB_SALL, true, 1, SZ_G2A);
  take(PB_FALL, true, 1, SZ_FP12);
  take(PB_MFLAG, true, 2, 1);  // [0] merged check passed, [1] constant 0 (req_bad of the merged pair)
  take(PB_MSTATS, true, 2, 4);
  // bucket MSM: keys + sorted entries, histogram / offsets / chunk offsets / cursors, chunk
  // partials, bucket sums, G_p
  take(PB_MKEYS, p.use_msm, p.n_ent, 4);
  take(PB_MSORTED, p.use_msm, p.n_ent, 4);
  take(PB_MHIST, p.use_msm, 4 * (LB_MSM_BUCKETS + 1), 4);
  take(PB_MCSUM, p.use_msm, p.max_chunks, SZ_G2J);
  take(PB_MBSUM, p.use_msm, LB_MSM_BUCKETS, SZ_G2J);
  take(PB_MG, p.use_msm, LB_MSM_POS, SZ_G2J);
  // steps organisation: size histogram + cursors, gt, row offsets, order, meta, G, split parts
  take(PB_RHIST, p.steps, 2 * (ns + 1), 4);
  take(PB_RGT, p.steps, ns + 1, 4);
  take(PB_ROWOFF, p.steps, ns + 1, 4);
  take(PB_RPOS, p.steps, nr, 4);
  take(PB_RINV, p.steps, nr, 4);
  take(PB_RMETA, p.steps, 1, 4);
  take(PB_G, p.steps, 144 * ns * p.lsplit, 4);
  take(PB_FPARTS, p.steps && p.lsplit > 1, nr1 * p.lsplit, SZ_FP12);
  take(PB_DEC_IN, p.dec_sets, (size_t)p.dec_sets * 4 * 16, 4);
  take(PB_DEC_FL, p.dec_sets, (size_t)p.dec_sets * 3, 4);
  take(PB_DEC_OUT, p.dec_sets, (size_t)p.dec_sets * 2 * 16, 4);
  take(PB_DEC_OFL, p.dec_sets, (size_t)p.dec_sets * 2, 4);
  take(PB_DEC_PRE, p.dec_sets, p.dec_sets, 1);
  take(PB_HF_IN, p.hf_sets, (size_t)p.hf_sets * 12 * 16, 4);
  take(PB_HF_OUT, p.hf_sets, (size_t)p.hf_sets * 6 * 16, 4);
  take(PB_LL_IN, p.ll_sets, (size_t)p.ll_sets * 9 * 16, 4);
  take(PB_LL_OUT, p.ll_sets, (size_t)p.ll_sets * LB_LP_LINES_NOUT * 16, 4);
  take(PB_PL, p.steps, LB_MTAIL_LEVELS, SZ_FP12);
  take(PB_LVA, p.level_wc, 63 * (size_t)p.lvl_per, SZ_FP12);
  take(PB_LVB, p.level_wc, 63 * (size_t)((p.lvl_per + LB_LVL_GROUP - 1) / LB_LVL_GROUP), SZ_FP12);
  take(PB_LHA, p.level_wc, 63 * (size_t)p.lvl_per, 1);
  take(PB_LHB, p.level_wc, 63 * (size_t)p.lvl_per, 1);
  take(PB_MT_IN, p.mtail, (size_t)LB_MTAIL_NIN * 16, 4);
  take(PB_MT_OUT, p.mt_out, 12 * 16, 4);
  take(PB_MB_IN0, p.bits_lp, (size_t)LB_MSM_BITS_INST * LB_MSM_BITS_GROUP * 6 * 16, 4);
  take(PB_MB_IN1, p.bits_lp, (size_t)LB_MSM_BITS_INST * 6 * 16, 4);
  take(PB_MB_IN2, p.bits_lp, (size_t)LB_MSM_BITS_INST / 8 * 6 * 16, 4);
  // the pair-major accumulation's late buffers: the folded merged pair's value, a split's halves
  take(PB_FX, p.fx, 1, SZ_FP12);
  take(PB_OFF2, p.halves, 2 * nr + 1, 4);
  take(PB_ACC_F, p.halves, 2 * nr, SZ_FP12);
  take(PB_ACC_BAD, p.halves, 2 * nr, 1);
  take(PB_ACC_ERR, p.halves, 2 * nr, 1);
  take(PB_PARTIAL, p.partial, 1, SZ_FP12);  // a two-phase call's merged Miller product, encoded (LB_GT_BYTES)
  L.bytes = at - start;
  return L;
}

}  // namespace lb
