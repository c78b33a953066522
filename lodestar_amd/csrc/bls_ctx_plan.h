// Planning of a context (bls_host.hip create_ctx), as host arithmetic: plain C++17, no HIP, so
// the rules and the queue guard are testable without a GPU (tests/native/ctx_plan_host.cpp).
//
//   CtxConfig      the context-level switches (LB_* environment, ctx_config_from_env)
//   DeviceFacts    what the plan needs to know of the device
//   QueueTally     streams by kind: the process's live ones, and what a context adds
//   plan_context   every decision of a context: slots, streams per slot, the CU mask, which
//                  stream each (slot, index) creates or shares, the hardware queues all of them
//                  take -- or the refusal of a configuration that must not run
//
// create_ctx gathers the facts, plans, and creates exactly the streams of the plan; lb_destroy
// releases them by the same plan.  Nothing below the plan reads a switch.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

namespace lb {

// ---- the switches -----------------------------------------------------------------------
struct CtxConfig {
  // One single-stream slot per hardware queue HIP gives this process: GPU_MAX_HW_QUEUES as
  // atoi reads it (0: unset; HIP's default is 4).  A host that sets 8 before HIP starts gets
  // 8 calls in flight: 2.94 vs 2.74 M sets/s once the merged check's one-wave kernels left
  // each call's queue idle at its end (profiles/ab_r03/hwq); up to kCtxMaxSlots.  More
  // streams than queues share a queue and measured -20 % (profiles/ab_r01i.txt).
  int max_hw_queues = 0;
  int slots = 0;          // LB_SLOTS: overrides the slot count when in 1 .. kCtxMaxSlots
  int slot0_streams = 0;  // LB_SLOT0_STREAMS=1|2 overrides slot 0's streams (the synchronous, lowest-latency slot)
  // The priority lane's CU reservation.  A running workgroup is never
  // preempted and a priority stream only reorders dispatch, so under load a latency-path
  // call would wait for a whole CU to drain.  LB_PRIO_CUS=K (-1, unset: 64 of at least 128;
  // 0 = off): masked streams that leave the K highest-numbered CUs to the priority lane.
  // LB_PRIO_DYN (default 1): throughput calls take them only while the priority lane has
  // been used within the last LB_PRIO_HOLD_MS (default 250), the full streams otherwise,
  // so a GPU without priority traffic keeps every CU.  Measured (profiles/r04/prio_ab/,
  // legs_ab/): 1-set / 128-set p50 under 16 calls in flight 1.2x / 1.9x idle (4-6x without),
  // C2 throughput unchanged.
  int prio_cus = -1;
  // LB_PRIO_SPREAD=1: the K reserved CUs evenly spaced over the CU ids instead (measured
  // worse: the mask bits do not map to CUs that way)
  bool prio_spread = false;
  bool prio_dyn = true;
  double prio_hold_ms = 250.0;
  // every masked stream takes a hardware queue of a pool of its own, and every queue
  // reserves scratch (§5.1): with LB_PRIO_DYN_SLOTS=K only the first K slots get one
  // masked stream each; while the priority lane is in use new calls go to those slots
  // (default 2: 16 + 16 ran out of scratch, like 24 queues of one pool; with 4 masked
  // queues the queues of a second context or process on the same GPU -- bench.py's
  // single-stream timing context, its node leg -- slowed every later call by a third,
  // with 2 they did not)
  int prio_dyn_slots = 2;
  // LB_TAIL_PRIO=1: one shared high-priority stream for every slot's merged check; off by
  // default, measured 2.40-2.43 vs 2.56-2.57 M sets/s (profiles/ab_r02s/r02s_d_*.json)
  bool tail_prio = false;
  double scratch_budget_gb = -1.0;  // LB_SCRATCH_BUDGET_GB (-1, unset: kBudgetQueues queues' worth)
  // same-message packages of at most LB_SM_DEC_MAX signatures decode them as round programs
  // (k_lp_dec; LB_SM_LP_DECODE=0: k_decode_sigs always)
  bool sm_lp_decode = true;
  bool sm_randomized = false;  // LB_SM_RANDOMIZED=1: the context starts in LB_SM_RANDOMIZED (lb_set_same_message_mode)
  uint32_t tp_pause = 32;      // LB_TP_PAUSE: two-phase calls in the legacy mode after a failed combine (0: always release)
  bool fault_rerun = false;    // LB_FAULT_RERUN=1 (tests only): a failed combine's re-run fails to submit
  bool gt_lp = true;       // lb_gt_check's final exponentiation as a round program (LB_GT_LP=0: one wave)
  bool prio_kcopy = true;  // the priority slot's host copies as kernels (slot_copy, LB_PRIO_KCOPY)
  // LB_DAG=0: a call never borrows a second stream (every kernel of a lone call runs
  // alone on the GPU: bench.py's per-kernel iso timings and their rocprof profile)
  bool dag = true;
  // LB_STAGE_EVENTS=0: no per-stage timing events (two HIP calls per kernel of the
  // submission; the N-API addon sets it, lb_last_stage_times is then empty)
  bool stage_events = true;
};

enum CtxEnvKind : uint8_t {
  CENV_FLAG,        // atoi(v) != 0
  CENV_IS_ONE,      // atoi(v) == 1
  CENV_INT,         // atoi(v)
  CENV_NONNEG,      // atoi(v); a negative value acts as 0
  CENV_ONE_ELSE_2,  // LB_SLOT0_STREAMS: 1 only for "1", else 2
  CENV_U32_ATOI,    // (uint32_t)atoi(v)
  CENV_DOUBLE,      // atof(v)
  CENV_NONNEG_D,    // atof(v); a negative value acts as 0
};
struct CtxEnvKnob {
  const char* name;
  CtxEnvKind kind;
  bool CtxConfig::*b;
  int CtxConfig::*i;
  uint32_t CtxConfig::*u;
  double CtxConfig::*d;
};
inline constexpr CtxEnvKnob cenv_b(const char* n, CtxEnvKind k, bool CtxConfig::*f) { return {n, k, f, nullptr, nullptr, nullptr}; }
inline constexpr CtxEnvKnob cenv_i(const char* n, CtxEnvKind k, int CtxConfig::*f) { return {n, k, nullptr, f, nullptr, nullptr}; }
inline constexpr CtxEnvKnob cenv_u(const char* n, CtxEnvKind k, uint32_t CtxConfig::*f) { return {n, k, nullptr, nullptr, f, nullptr}; }
inline constexpr CtxEnvKnob cenv_d(const char* n, CtxEnvKind k, double CtxConfig::*f) { return {n, k, nullptr, nullptr, nullptr, f}; }

static constexpr CtxEnvKnob kCtxEnvKnobs[] = {
    cenv_i("GPU_MAX_HW_QUEUES", CENV_INT, &CtxConfig::max_hw_queues),
    cenv_i("LB_SLOTS", CENV_INT, &CtxConfig::slots),
    cenv_i("LB_SLOT0_STREAMS", CENV_ONE_ELSE_2, &CtxConfig::slot0_streams),
    cenv_i("LB_PRIO_CUS", CENV_NONNEG, &CtxConfig::prio_cus),
    cenv_b("LB_PRIO_SPREAD", CENV_IS_ONE, &CtxConfig::prio_spread),
    cenv_b("LB_PRIO_DYN", CENV_FLAG, &CtxConfig::prio_dyn),
    cenv_d("LB_PRIO_HOLD_MS", CENV_DOUBLE, &CtxConfig::prio_hold_ms),
    cenv_i("LB_PRIO_DYN_SLOTS", CENV_INT, &CtxConfig::prio_dyn_slots),
    cenv_b("LB_TAIL_PRIO", CENV_IS_ONE, &CtxConfig::tail_prio),
    cenv_d("LB_SCRATCH_BUDGET_GB", CENV_NONNEG_D, &CtxConfig::scratch_budget_gb),
    cenv_b("LB_SM_LP_DECODE", CENV_FLAG, &CtxConfig::sm_lp_decode),
    cenv_b("LB_SM_RANDOMIZED", CENV_IS_ONE, &CtxConfig::sm_randomized),
    cenv_u("LB_TP_PAUSE", CENV_U32_ATOI, &CtxConfig::tp_pause),
    cenv_b("LB_FAULT_RERUN", CENV_FLAG, &CtxConfig::fault_rerun),
    cenv_b("LB_GT_LP", CENV_FLAG, &CtxConfig::gt_lp),
    cenv_b("LB_PRIO_KCOPY", CENV_FLAG, &CtxConfig::prio_kcopy),
    cenv_b("LB_DAG", CENV_FLAG, &CtxConfig::dag),
    cenv_b("LB_STAGE_EVENTS", CENV_FLAG, &CtxConfig::stage_events),
};

// Apply the environment (`lookup`: getenv, or a test's table) to the defaults in `c`.
inline void ctx_config_from_env(CtxConfig& c, const char* (*lookup)(const char*)) {
  for (const CtxEnvKnob& k : kCtxEnvKnobs) {
    const char* v = lookup(k.name);
    if (!v) continue;
    switch (k.kind) {
      case CENV_FLAG: c.*k.b = atoi(v) != 0; break;
      case CENV_IS_ONE: c.*k.b = atoi(v) == 1; break;
      case CENV_INT: c.*k.i = atoi(v); break;
      case CENV_NONNEG: c.*k.i = atoi(v) > 0 ? atoi(v) : 0; break;
      case CENV_ONE_ELSE_2: c.*k.i = atoi(v) == 1 ? 1 : 2; break;
      case CENV_U32_ATOI: c.*k.u = (uint32_t)atoi(v); break;
      case CENV_DOUBLE: c.*k.d = atof(v); break;
      case CENV_NONNEG_D: c.*k.d = atof(v) > 0 ? atof(v) : 0.0; break;
    }
  }
}

// ---- the device and the process ---------------------------------------------------------
struct DeviceFacts {
  int cus = 0;              // compute units (0: unknown)
  uint32_t lane_bytes = 0;  // the largest private segment of the library's kernels, bytes per lane
};

// Private-segment (scratch) reservation of one HIP hardware queue.  ROCr backs a queue's
// scratch for a dispatch at full-device occupancy: private bytes per lane x 64 lanes x 32
// waves per CU x CUs (256 where the count is unknown), and keeps it for the queue's lifetime,
// so a process with Q queues that run the pipeline's largest-scratch kernel reserves Q times
// that.  At 24 queues the first 65,536-set calls failed with HSA_STATUS_ERROR_OUT_OF_RESOURCES
// (profiles/ab_r03/r03g_q24_fail.txt) with the HBM otherwise free; 16 ran,
// which is the cap plan_context enforces.
inline int budget_cus(const DeviceFacts& d) { return d.cus ? d.cus : 256; }
inline size_t queue_scratch_bytes(const DeviceFacts& d) { return (size_t)d.lane_bytes * 64 * 32 * (size_t)budget_cus(d); }

// Streams by kind: HIP pools the plain streams of one priority into at most
// GPU_MAX_HW_QUEUES queues PER PROCESS, so a second context's plain and high-priority streams
// share the first one's queues (up to that cap) while each CU-masked stream takes a queue of
// its own.
struct QueueTally {
  int plain = 0, high = 0, masked = 0;
};
inline int pooled_queues(const QueueTally& t, int maxq) {
  return (t.plain < maxq ? t.plain : maxq) + (t.high < maxq ? t.high : maxq) + t.masked;
}

constexpr int kCtxMaxSlots = 16;
// the largest configuration that ran: 16 plain + 2 masked + 2 high-priority queues at 3,328
// private bytes per lane; 24 + 2 plain (r03) and 16 + 16 masked + 2 (r04) queues failed with
// HSA_STATUS_ERROR_OUT_OF_RESOURCES
constexpr int kBudgetQueues = 20;
constexpr int kBudgetLaneBytes = 3328;
// A latency-lane context (lb_create_lane, optional: the addon runs without one) is priced on
// the process total, the largest process configuration seen to run: bench.py's process and the
// node addon's, 16 plain + 2 CU-masked + 4 high-priority queues (the main context's priority
// lane and aux stream, and the second context's two).
constexpr int kProcessQueueBudget = 22;

// ---- the plan ---------------------------------------------------------------------------
enum StreamKind : uint8_t {
  ST_NONE,    // no such stream
  ST_OWN,   // its own: hipStreamCreateWithFlags (Slot::st_full), hipExtStreamCreateWithCUMask (st_mask)
  ST_HIGH,    // its own, at the device's highest priority (st_full of the priority lane)
  ST_ALIAS0,  // the slot's stream 0 of the same pair
};
// What creation does for stream `i` of a slot: the stream without the CU mask, the one with it,
// and which of the two Slot::st[i] starts as (pick_streams switches a dynamic slot's later).
struct StreamPlan {
  StreamKind full = ST_NONE, mask = ST_NONE;
  bool starts_masked() const { return full == ST_NONE; }
};
inline bool owned(StreamKind k) { return k == ST_OWN || k == ST_HIGH; }

struct CtxPlan {
  bool lane = false;  // lb_create_lane: a latency-lane context (one slot, no CU-masked streams)
  int n_slots = 4;
  int streams_per_slot[kCtxMaxSlots + 1] = {};  // [n_slots]: the priority lane
  std::vector<uint32_t> cu_mask;                // the throughput streams' CUs (empty: no reservation)
  int prio_cus = 0;                             // CUs the throughput slots leave to the priority lane
  // the throughput calls take the masked streams only while the priority lane has been used
  // within the last prio_hold_ms; slots [0, prio_dyn_slots) own masked streams
  bool prio_dyn = false;
  int prio_dyn_slots = 0;
  double prio_hold_ms = 250.0;
  StreamPlan st[kCtxMaxSlots + 1][2];
  int mask_slot[kCtxMaxSlots] = {};  // the slot whose masked streams slot s queues on while the lane is in use
  bool tail_stream = false;
  // the streams this context adds to the process tally (the priority lane, lb_gt_check's aux
  // stream and the tail stream are the high-priority ones), and the hardware queues they take
  int q_plain = 0, q_high = 0, q_masked = 0;
  int hw_queues = 0;
  int err = 0;  // LB_ERR_RESOURCES: refused, nothing may be created; msg says why
  char msg[400] = {};
};

constexpr int kCtxErrResources = -5;  // (LB_ERR_RESOURCES, include/lodestar_bls.h)

// `live`: the streams of every live context of this process (the caller holds their lock until
// it has added this plan's).
inline CtxPlan plan_context(const CtxConfig& c, const DeviceFacts& dev, bool lane, const QueueTally& live) {
  CtxPlan p;
  p.lane = lane;
  const size_t per_q = queue_scratch_bytes(dev);
  if (c.max_hw_queues > kCtxMaxSlots) {
    snprintf(p.msg, sizeof p.msg,
             "GPU_MAX_HW_QUEUES=%d exceeds %d: %u private bytes per lane reserve %.2f GB of scratch per "
             "hardware queue (%.1f GB for %d queues); 24 queues failed with HSA_STATUS_ERROR_OUT_OF_RESOURCES",
             c.max_hw_queues, kCtxMaxSlots, dev.lane_bytes, per_q / 1e9, per_q * (double)c.max_hw_queues / 1e9,
             c.max_hw_queues);
    p.err = kCtxErrResources;
    return p;
  }
  // slots and their streams
  p.n_slots = c.max_hw_queues < 4 ? 4 : c.max_hw_queues;
  if (c.slots >= 1 && c.slots <= kCtxMaxSlots) p.n_slots = c.slots;
  if (lane) p.n_slots = 1;  // its priority lane (+ one slot for helpers)
  const int n = p.n_slots;
  for (int s = 0; s < n; s++) p.streams_per_slot[s] = lane ? 1 : n <= 2 ? 2 : (n == 3 && s == 0) ? 2 : 1;
  p.streams_per_slot[n] = 1;
  if (c.slot0_streams) p.streams_per_slot[0] = c.slot0_streams;
  // the CU mask (the reservation belongs to the throughput context: lb_mark_priority)
  const int k = lane ? 0 : c.prio_cus >= 0 ? c.prio_cus : dev.cus >= 128 ? 64 : 0;
  if (k > 0 && k < dev.cus) {
    p.cu_mask.assign((size_t)(dev.cus + 31) / 32, 0u);
    std::vector<char> reserved((size_t)dev.cus, 0);
    for (int j = 0; j < k; j++)
      reserved[c.prio_spread ? (size_t)((int64_t)(j + 1) * dev.cus / k - 1) : (size_t)(dev.cus - k + j)] = 1;
    for (int cu = 0; cu < dev.cus; cu++)
      if (!reserved[cu]) p.cu_mask[cu / 32] |= 1u << (cu % 32);
    p.prio_cus = k;
    p.prio_dyn = c.prio_dyn;
    p.prio_hold_ms = c.prio_hold_ms;
    p.prio_dyn_slots = p.prio_dyn && c.prio_dyn_slots >= 1 && c.prio_dyn_slots < n ? c.prio_dyn_slots : n;
  }
  const bool mask = !p.cu_mask.empty();
  const bool one = p.prio_dyn && p.prio_dyn_slots < n;  // one masked stream per owning slot
  // every stream: a slot has its full streams unless every call is masked, and masked ones if it owns any
  for (int s = 0; s <= n; s++) {
    for (int i = 0; i < 2; i++) {
      StreamPlan& e = p.st[s][i];
      if (i >= p.streams_per_slot[s]) {  // a single-stream slot: both entries are the one stream
        e.full = p.st[s][0].full == ST_NONE ? ST_NONE : ST_ALIAS0;
        e.mask = p.st[s][0].mask == ST_NONE ? ST_NONE : ST_ALIAS0;
      } else if (s == n) {
        e.full = ST_HIGH;
      } else {
        e.full = !mask || p.prio_dyn ? ST_OWN : ST_NONE;
        e.mask = !mask || s >= p.prio_dyn_slots ? ST_NONE : one && i > 0 ? ST_ALIAS0 : ST_OWN;
      }
      p.q_plain += e.full == ST_OWN;
      p.q_high += e.full == ST_HIGH;
      p.q_masked += e.mask == ST_OWN;
    }
    // a slot without masked streams queues on those of slot (s mod K) -- on the GPU, not in
    // finish_slot: the submitting thread never waits longer than the round robin makes it
    if (s < n) p.mask_slot[s] = mask ? s % p.prio_dyn_slots : s;
  }
  p.tail_stream = c.tail_prio;
  p.q_high += 1 + (p.tail_stream ? 1 : 0);  // lb_gt_check's aux stream, the tail stream
  // Every hardware queue this context opens reserves scratch for the largest private
  // segment it runs: price all of them, not only GPU_MAX_HW_QUEUES
  // (VERDICT r4 #7).
  const int maxq = c.max_hw_queues > 0 ? c.max_hw_queues : 4;
  const QueueTally add{p.q_plain, p.q_high, p.q_masked};
  p.hw_queues = pooled_queues(add, maxq);
  const int cus = budget_cus(dev);
  const double budget = c.scratch_budget_gb >= 0 ? c.scratch_budget_gb * 1e9
                                                 : (double)kBudgetQueues * kBudgetLaneBytes * 64 * 32 * cus;
  if ((double)per_q * p.hw_queues > budget) {
    snprintf(p.msg, sizeof p.msg,
             "%d hardware queues (%d plain of GPU_MAX_HW_QUEUES=%d, %d CU-masked, %d high-priority) x %u private "
             "bytes per lane x 64 x 32 x %d CUs = %.1f GB of scratch exceeds the %.1f GB budget (20 queues at "
             "3,328 B/lane ran; 16 + 16 masked failed with HSA_STATUS_ERROR_OUT_OF_RESOURCES)",
             p.hw_queues, p.q_plain < maxq ? p.q_plain : maxq, maxq, p.q_masked, p.q_high < maxq ? p.q_high : maxq,
             dev.lane_bytes, cus, per_q * (double)p.hw_queues / 1e9, budget / 1e9);
    p.err = kCtxErrResources;
    return p;
  }
  const QueueTally proc{live.plain + p.q_plain, live.high + p.q_high, live.masked + p.q_masked};
  if (lane && pooled_queues(proc, maxq) > kProcessQueueBudget) {
    snprintf(p.msg, sizeof p.msg,
             "latency-lane context refused: the process would hold %d hardware queues (%d plain, %d high-priority "
             "streams pooled into at most GPU_MAX_HW_QUEUES=%d each, %d CU-masked), above the %d that ran",
             pooled_queues(proc, maxq), proc.plain, proc.high, maxq, proc.masked, kProcessQueueBudget);
    p.err = kCtxErrResources;
  }
  return p;
}

}  // namespace lb
