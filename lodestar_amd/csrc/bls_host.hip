// MI355X (gfx950) BLS12-381 signature-set verification pipeline + C ABI.
//
// One lane per signature set for the per-set stages; one workgroup per set
// for pubkey aggregation; one lane per request for the request reductions.
// Integer VALU only (v_mad_u64_u32 chains); see DESIGN.md for the roofline.
//
// Pipeline of lb_verify_requests (reference: BlsMultiThreadWorkerPool job ->
// worker verifyManySignatureSets -> verifySignatureSetsMaybeBatch,
// packages/beacon-node/src/chain/bls/multithread/worker.ts:30-108,
// chain/bls/maybeBatch.ts:16-46).  A call is planned (bls_plan.h: every decision and the
// workspace layout, plain host arithmetic), then enqueued stage by stage (run_pipeline);
// the default organisation of a throughput call, "steps":
//   k_req_flags, k_rows_*  per request : 1-set requests need core-verify checks; the
//                                        size-descending order and row offsets of the lanes
//   k_pubkeys_*            per set     : PublicKey.fromBytes + PublicKey.aggregate
//   k_scalar_pk            per set     : r_i pk_i (GLV, 2 x 32-bit)
//   k_hash_half/finish     per message : hash_to_G2(signing root), two lanes per message
//   k_lines_rows           per set     : the 68 lines of (r_i pk_i, H_i), stored
//   k_decode_sigs          per set     : Signature.fromBytes(validate=true)
//   k_req_status           per request : rejection codes, bad requests
//   k_msm_*                per call    : S_all = sum r_i sig_i over the good requests, one
//                                        bucket MSM (k_msm.hip); small calls: per-set ladders
//                                        (k_scalar_sig + k_sum_tree), also the S_k of the tails
//   k_step_acc             per set     : step-major lanes over the stored lines (k_steps.hip;
//                                        from 8,192 sets k_line_pairs multiplies their line pairs first)
//   k_level_part/_wc       per call    : the 63 level products of the merged check
//   k_lp_mtail             per call    : merged check as a round program: S_all from the MSM's
//                                        bit sums, Miller(-g1, S_all), Horner chain, final exp
//   k_req_horner + k_lp_rtail per request, only after a failed merged check: F_k,
//                                        Miller(-g1, S_k), final exponentiation, == 1
// A lone mid-size call runs hash finish, decode and lines as round programs (k_lp_*); the
// pairs organisation (LB_ACC=pairs: k_lines + k_miller_acc, several pairs per lane), the
// per-set Miller loops of small calls (k_miller_sets / k_pair_wc + k_prod_tree) and the
// one-wave tails (k_lines_S + k_tail) remain selectable; calls of at most 1,024 sets take
// the latency path (run_lp, k_lp.hip) instead.  DESIGN.md §4.5-4.6.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdlib>
#include <mutex>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "bls_kernels.h"
#include "bls_kzg.h"
#include "bls_lp.h"
#include "bls_ctx_plan.h"
#include "bls_plan.h"
#ifdef LB_LP_PROGS_HEADER  // (a variant's programs, tools/lp_rows_variant.py)
#include LB_LP_PROGS_HEADER
#else
#include "bls_lp_progs.h"
#endif

using namespace lb;

// the latency path's round programs (gen_lp.py), embedded by lp_blob.hip
extern "C" const uint32_t lb_lp_blob[];

#ifdef LB_COUNT_OPS
static unsigned long long opcount_read_reset() {
  unsigned long long v = 0, z = 0;
  (void)hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_lb_fpmul_count), sizeof(v));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_lb_fpmul_count), &z, sizeof(z));
  return v;
}
#endif

// ============================================================================
// Host side: context, workspace, C ABI
// ============================================================================
// What a call keeps between its front half (everything up to the merged
// product) and its tails (per-request final exponentiations), so a two-phase
// call (lb_verify_requests_partial_async) can stop after the front half, hand
// its Fp12 partial to the host and resume with the host's combined verdict.
struct PipeState {
  uint32_t n_req = 0, n_sets = 0, n_pairs = 0;
  bool merged = false, tail_wave = true;
  // merged check's S_all from the bucket MSM: the per-request S_k (per-set
  // ladders + sums) are computed only when the tails run
  bool msm = false;
  const uint8_t* d_seed = nullptr;
  const g2j* d_sig = nullptr;
  const uint8_t* d_sig_st = nullptr;
  g2j* d_rsig = nullptr;
  const uint32_t* d_req_off = nullptr;
  uint32_t* d_lines = nullptr;
  g2a* d_S = nullptr;
  fp12* d_F = nullptr;
  uint8_t* d_bad = nullptr;
  uint8_t* d_valid = nullptr;
  uint8_t* d_mflag = nullptr;
  uint32_t* d_mstats = nullptr;
  // steps organisation of the Miller accumulation (k_steps.hip): the lanes'
  // level products G (per-request F_k only when the tails need them)
  bool steps = false;
  Rows rows{};
  const uint32_t* d_G = nullptr;
  fp12* d_Fparts = nullptr;  // (a split accumulation: k_req_horner's parts per request, k_req_join)
  // the failed merged check's per-request tails as round programs (k_lp_rtail): staged inputs
  uint32_t* d_rt_in = nullptr;
  uint32_t* d_rt_fl = nullptr;
};

// A same-message package in flight (lb_verify_same_message_batch[_async]):
// what its completion needs after phase 1 (the jobs' aggregated sets) to
// publish verdicts and, for failed jobs, to run phase 2 (every set of those
// jobs alone) on the same slot from the device-resident decoded signatures.
struct SmState {
  bool active = false;
  int phase = 0;                     // 1: phase 1 in flight, 2: phase 2 (retries) in flight
  uint32_t nr = 0, retried_jobs = 0, fast_sets = 0;
  uint32_t mode = LB_SM_PLAIN;       // the context's aggregation mode when the package was submitted
  uint32_t nj = 0, ns = 0;
  uint8_t* out_valid = nullptr;     // caller: n_sets verdicts
  uint8_t* out_job_fast = nullptr;  // caller (optional): n_jobs flags
  // the package's buffers of both phases -- device-resident inputs and decoded signatures, the
  // pinned result rows and retry lists -- as offsets of the slot's slab and staging (bls_carve.h)
  SmShape shape;
  SmLayout lay;
  // lb_verify_same_message_batch_agg: the jobs' aggregate signatures (sm_job_sig, k_aggsig.hip)
  bool agg = false, masked = false;  // (masked: the caller passed a mask)
  uint8_t* out_job_sig96 = nullptr;  // caller: n_jobs x 96
  uint32_t* out_job_count = nullptr; // caller: n_jobs
  int err = 0;                       // a failed phase-2 launch: reported by this ticket's wait
  std::string err_msg;
};

// One in-flight call: two streams (DAG), own workspace, staging and events.
struct Slot {
  hipStream_t st[2] = {};
  // the slot's streams without and with the CU mask, as the context's plan has them
  // (bls_ctx_plan.h StreamPlan); st[] is one pair or the other, chosen when a call is
  // submitted (pick_streams, LB_PRIO_DYN)
  hipStream_t st_full[2] = {}, st_mask[2] = {};
  hipEvent_t dep[8] = {};
  hipEvent_t done = nullptr;
  char* d_ws = nullptr;
  size_t ws_cap = 0;
  char* h_pin = nullptr;
  size_t pin_cap = 0;
  // (32 launches of the longest pipeline call, and room for what an _agg same-message call adds behind it)
  static constexpr int kMaxStages = 40;
  hipEvent_t ev0[kMaxStages] = {}, ev1[kMaxStages] = {};
  const char* stage_name[kMaxStages] = {};
  int n_stages = 0;
  unsigned long long stage_ops[kMaxStages] = {};
  hipEvent_t wall0 = nullptr, wall1 = nullptr;
  bool busy = false;
  uint64_t ticket = 0;
  uint32_t* h_stats = nullptr;  // pinned: [batch_retries, batch_sigs_success] of the call in flight
  PipeState ps;
  // two-phase calls: front half enqueued, tails wait for lb_verify_requests_finish
  bool partial_pending = false;
  hipEvent_t partial_ev = nullptr;
  uint8_t* h_partial = nullptr;  // pinned, 576 B
  // host-buffer calls: device outputs, their pinned copies and the caller's
  // buffers they are copied into when the call retires (finish_slot)
  uint8_t *dv_valid = nullptr, *dv_err = nullptr, *dv_sst = nullptr;
  uint8_t *hv_valid = nullptr, *hv_err = nullptr, *hv_sst = nullptr;
  uint8_t *out_valid = nullptr, *out_err = nullptr, *out_sst = nullptr;
  uint32_t out_nr = 0, out_ns = 0;
  SmState sm;
  // an async call on an otherwise idle GPU runs as the two-stream DAG with the
  // stream of an idle slot (borrowed); that slot is lent (busy) until the call retires
  Slot* borrowed = nullptr;
  Slot* lent_to = nullptr;
  // a synchronous call's second stream (borrow_second_stream): pick_streams keeps it
  hipStream_t guard_st = nullptr;
  // latency-path calls: the kernel's clock stamps (pinned, LpCall::clk), published to
  // ctx->lp_clk when the call retires
  unsigned long long* h_clk = nullptr;
  bool lp_call = false;
};

// The context's last error message.  lb_gt_check may run on one thread while another
// submits and retires calls (include/lodestar_bls.h), and both can fail: every write
// and read of the message takes a lock.
class ErrorText {
 public:
  ErrorText& operator=(std::string v) {
    std::lock_guard<std::mutex> g(mu_);
    s_ = std::move(v);
    return *this;
  }
  operator std::string() const {
    std::lock_guard<std::mutex> g(mu_);
    return s_;
  }

 private:
  mutable std::mutex mu_;
  std::string s_;
};

// A released two-phase call (LB_TP_RELEASE): what lb_partial_wait, lb_verify_requests_finish
// and lb_wait need once its slot has moved on -- the partial, and the call itself (the
// caller's buffers stay valid until lb_wait returns) for a re-run when the combine fails.
// Until its ticket is waited for, a released call's outputs hold provisional verdicts (every
// request not already false valid), so a record is never overwritten while it can still
// change them: lb_verify_requests_partial_async refuses a call whose ring entry is live
// (tp_reusable).  `failed`: the re-run after a failed combined check could not be submitted;
// lb_wait then returns that error instead of the provisional verdicts.
struct TwoPhaseRec {
  uint64_t ticket = 0;
  bool device = false, finished = false, have_partial = false, failed = false, waited = false;
  uint64_t rerun = 0;  // the one-phase re-run's ticket (failed combine)
  lb_request_batch batch{};
  // (a lb_verify_requests_keys_partial_async call: its key source, for the same re-run)
  bool by_keys = false;
  lb_key_source keys{};
  uint8_t *valid = nullptr, *err = nullptr, *sst = nullptr;
  uint8_t partial[LB_GT_BYTES];
};

// Stats of a retired call, kept per ticket (lb_wait reports the stats of ITS
// ticket even when another call retired the slot first).
struct TicketStats {
  uint64_t ticket = 0;
  uint32_t batch_retries = 0, batch_sigs_success = 0;
  float wall_ms = 0.f;
};

// A device array the context owns for its lifetime: d[0, n) of cap entries.  reserve() makes
// room for `need` entries by the array's policy (dev_array_cap, bls_carve.h), keeps the first
// `keep` (n = keep once the array has moved) and names the array in the context's error when
// the device has no room.  The calls in flight, which may read the array, are the caller's to
// retire first (helper_slot), and the copies are the caller's to wait for.
struct lb_ctx;
template <class T>
struct DevArray {
  const char* const name;
  const uint32_t floor;
  const bool doubling;
  T* d = nullptr;
  uint32_t n = 0, cap = 0;
  explicit DevArray(const char* name_, uint32_t floor_ = 0, bool doubling_ = false)
      : name(name_), floor(floor_), doubling(doubling_) {}
  DevArray(const DevArray&) = delete;
  DevArray& operator=(const DevArray&) = delete;
  ~DevArray() {
    if (d) (void)hipFree(d);
  }
  int reserve(lb_ctx* ctx, uint32_t need, uint32_t keep);
  // d[first, first + count) from / to host memory, on ctx->stream
  int upload(lb_ctx* ctx, uint32_t first, const T* src, uint32_t count);
  int download(lb_ctx* ctx, uint32_t first, T* dst, uint32_t count) const;
};

// Blob KZG (lb_kzg_*): what persists across calls -- the roots-of-unity table and the two
// halves of the loaded setup.  A call's own buffers are carved from slot 0's slab (HelperCall).
struct KzgState {
  bool loaded = false;
  DevArray<fr> roots{"KZG roots"};     // roots[i] = omega^brp(i), Montgomery form (k_kzg_roots); n: built
  DevArray<g2a> neg_tau{"KZG setup"};  // [0]: -[tau]_2 of the loaded setup, [1]: a candidate being checked
  // commitments and proofs (k_kzg_msm.hip): the window table of the Lagrange G1 setup,
  // T[j][i] = [2^(8j)] L[i]; [g1_cur] is the loaded one, the other takes a candidate
  bool g1_loaded = false;
  DevArray<g1a> g1_tab[2] = {DevArray<g1a>{"KZG G1 table"}, DevArray<g1a>{"KZG G1 table"}};
  int g1_cur = 0;
};

struct lb_ctx {
  int device = -1;
  KzgState kzg;
  // the context's switches and every decision taken from them at creation (bls_ctx_plan.h):
  // slots, streams, CU mask, hardware queues.  plan.n_slots calls are in flight on the async
  // API; a synchronous call runs on slot 0 as the two-stream DAG by borrowing slot 1's stream
  // for its duration.
  CtxConfig ccfg;
  CtxPlan plan;
  // slots[plan.n_slots] is the priority lane: one stream at the device's highest
  // priority, outside the async round robin, for latency-critical calls
  // (lb_verify_requests_priority_async, and lb_verify_requests of at most
  // lp_max_sets sets): they never queue behind the calls in flight
  Slot slots[kCtxMaxSlots + 1];
  Slot& prio() { return slots[plan.n_slots]; }
  // steady-clock ns of the priority lane's last use (or lb_mark_priority from another
  // thread: an atomic, the one field of a context another thread may write)
  std::atomic<int64_t> last_prio_ns{INT64_MIN / 2};
  int next_slot = 0;
  uint64_t next_ticket = 1;
  // the last tickets issued to two-phase calls: lb_verify_requests_finish accepts a
  // ticket whose call a slot reuse already resumed only if it is one of these
  static constexpr int kTwoPhaseRing = 256;
  uint64_t two_phase[kTwoPhaseRing] = {};
  int two_phase_pos = 0;
  // (LB_TP_RELEASE: cfg.tp_release / cfg.tp_release_cfg; one record per two-phase ticket, ring by ticket)
  uint32_t tp_pause = 0;  // two-phase calls still to run in the legacy mode (ccfg.tp_pause after a failed combine)
  TwoPhaseRec tp[kTwoPhaseRing];
  ErrorText err;
  hipStream_t stream = nullptr;  // slot 0 stream 0 (synchronous helper calls)
  // the switches that shape a pipeline call (bls_plan.h: plan_pipeline reads nothing else)
  PipeConfig cfg;
  // same-message aggregation of the packages submitted from now on: LB_SM_PLAIN (plain sums, the
  // reference snapshot's) or LB_SM_RANDOMIZED (sum s_i pk_i / sum s_i sig_i, k_smrand.hip);
  // lb_set_same_message_mode; ccfg.sm_randomized at lb_create
  uint32_t sm_mode = LB_SM_PLAIN;
  // device-resident pubkey table (index2pubkey mirror, lb_pubkey_table_*)
  DevArray<g1a> table{"pubkey table", 4096, true};
  // device-resident index lists (lb_index_list_*): shufflings and sync committees that the sets
  // of a lb_verify_requests_keys* call name their keys from (k_lists.hip); n stays 0 until the
  // kernels or the copy that fill a list are known to have run
  struct IndexList : DevArray<uint32_t> {
    IndexList() : DevArray("index list", 1024) {}
  } lists[LB_INDEX_LISTS];
  // device-resident balance table (EffectiveBalanceIncrements mirror, lb_balance_table_*): one
  // byte per validator, what lb_sample_by_balance weighs its candidates by (k_sample.hip)
  DevArray<uint8_t> bal{"balance table", 4096, true};
  // the stage clock of the synchronous helper calls (HelperCall::stage): stage i of a call spans
  // helper_ev[i] .. helper_ev[i + 1]
  static constexpr int kHelperStages = 4;
  hipEvent_t helper_ev[kHelperStages + 1] = {};
  // timing of the last completed verify call, or of the last helper call that timed its stages
  int n_stages = 0;
  float stage_ms[Slot::kMaxStages] = {};
  const char* stage_name[Slot::kMaxStages] = {};
  unsigned long long stage_ops[Slot::kMaxStages] = {};
  float wall_ms = 0.f;
  uint32_t batch_retries = 0, batch_sigs_success = 0;
  static constexpr int kTicketRing = 64;
  TicketStats tstats[kTicketRing];
  // lb_gt_check runs on its own stream and buffers, so the host combine of the
  // shards' partials never drains the slots' calls in flight
  hipStream_t aux_stream = nullptr;
  // the merged check's one-wave chain of every slot (highest priority) when
  // plan.tail_stream; nullptr (default): the slot's own stream
  hipStream_t tail_stream = nullptr;
  uint8_t* d_aux = nullptr;
  uint8_t* h_aux = nullptr;
  size_t aux_cap = 0;
  // latency path: the round programs in device memory (uploaded on first use);
  // calls of at most cfg.lp_max_sets sets run it instead of the throughput pipeline
  DevArray<uint32_t> d_lp{"latency-path programs"};
  int last_call_streams = 0;  // streams of the last submitted verify call (begin_call)
  unsigned long long lp_clk[4] = {};  // clock stamps of the last retired latency-path call
};

#define LB_HIP(call)                                                                   \
  do {                                                                               \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                    \
      return LB_ERR_DEVICE;                                                            \
    }                                                                                  \
  } while (0)

#define LB_TRY(x)                 \
  do {                            \
    int rc_ = (x);                \
    if (rc_ != LB_OK) return rc_; \
  } while (0)

template <class T>
int DevArray<T>::reserve(lb_ctx* ctx, uint32_t need, uint32_t keep) {
  if (need <= cap) return LB_OK;
  const uint32_t grown = dev_array_cap(cap, need, floor, doubling);
  T* fresh = nullptr;
  if (hipMalloc(&fresh, sizeof(T) * (size_t)grown) != hipSuccess) {
    ctx->err = std::string("hipMalloc ") + name + " failed";
    return LB_ERR_OUT_OF_MEMORY;
  }
  if (d) {  // (the old array stays as it is when the copy fails)
    hipError_t e = keep ? hipMemcpyAsync(fresh, d, sizeof(T) * (size_t)keep, hipMemcpyDeviceToDevice, ctx->stream)
                        : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      (void)hipFree(fresh);
      ctx->err = std::string("moving the ") + name + ": " + hipGetErrorString(e);
      return LB_ERR_DEVICE;
    }
    LB_HIP(hipFree(d));
  }
  d = fresh;
  cap = grown;
  n = keep;
  return LB_OK;
}
template <class T>
int DevArray<T>::upload(lb_ctx* ctx, uint32_t first, const T* src, uint32_t count) {
  LB_HIP(hipMemcpyAsync(d + first, src, sizeof(T) * (size_t)count, hipMemcpyHostToDevice, ctx->stream));
  return LB_OK;
}
template <class T>
int DevArray<T>::download(lb_ctx* ctx, uint32_t first, T* dst, uint32_t count) const {
  LB_HIP(hipMemcpyAsync(dst, d + first, sizeof(T) * (size_t)count, hipMemcpyDeviceToHost, ctx->stream));
  return LB_OK;
}

namespace {

inline uint32_t blocks_for(uint32_t n, uint32_t tpb = TPB) { return (n + tpb - 1) / tpb; }

// A slot's slab as a pipeline call finds it: `fill` bytes are taken by the caller's own buffers
// (bls_carve.h), run_pipeline lays its workspace out from there and moves the fill past it
struct Slab {
  char* base;
  size_t fill;
  size_t cap;
};
template <class T>
T* slab_at(char* base, size_t off) { return off == kCarveAbsent ? nullptr : reinterpret_cast<T*>(base + off); }

int ensure_ws(lb_ctx* ctx, Slot& sl, size_t bytes) {
  if (bytes <= sl.ws_cap) return LB_OK;
  if (sl.d_ws) {
    LB_HIP(hipStreamSynchronize(sl.st[0]));
    LB_HIP(hipStreamSynchronize(sl.st[1]));
    LB_HIP(hipFree(sl.d_ws));
    sl.d_ws = nullptr;
    sl.ws_cap = 0;
  }
  size_t cap = bytes + bytes / 4 + (1 << 20);
  if (hipMalloc(&sl.d_ws, cap) != hipSuccess) {
    ctx->err = "hipMalloc workspace failed";
    return LB_ERR_OUT_OF_MEMORY;
  }
  sl.ws_cap = cap;
  return LB_OK;
}
int ensure_ws(lb_ctx* ctx, size_t bytes) { return ensure_ws(ctx, ctx->slots[0], bytes); }

int ensure_pin(lb_ctx* ctx, Slot& sl, size_t bytes) {
  if (bytes <= sl.pin_cap) return LB_OK;
  if (sl.h_pin) {
    LB_HIP(hipStreamSynchronize(sl.st[0]));
    LB_HIP(hipHostFree(sl.h_pin));
    sl.h_pin = nullptr;
    sl.pin_cap = 0;
  }
  size_t cap = bytes + bytes / 4 + (1 << 20);
  if (hipHostMalloc(&sl.h_pin, cap, hipHostMallocDefault) != hipSuccess) {
    ctx->err = "hipHostMalloc staging failed";
    return LB_ERR_OUT_OF_MEMORY;
  }
  sl.pin_cap = cap;
  return LB_OK;
}

#ifdef LB_COUNT_OPS
#define LB_COUNT_SYNC() LB_HIP(hipDeviceSynchronize())
#define LB_COUNT_TAKE(i) sl.stage_ops[i] = opcount_read_reset()
#else
#define LB_COUNT_SYNC() ((void)0)
#define LB_COUNT_TAKE(i) ((void)0)
#endif

// Launch `kern` on stream `s` of slot `sl`, bracketed by timing events.
#define LB_STAGE_ON(name, strm, kern, grid, block, ...)                                    \
  do {                                                                                     \
    const int si_ = (ctx->ccfg.stage_events && sl.n_stages < Slot::kMaxStages) ? sl.n_stages++ : -1; \
    hipStream_t strm_ = (strm);                                                            \
    LB_COUNT_SYNC();                                                                       \
    if (si_ >= 0) {                                                                        \
      LB_COUNT_TAKE(si_);                                                                  \
      sl.stage_name[si_] = name;                                                           \
      LB_HIP(hipEventRecord(sl.ev0[si_], strm_));                                          \
    }                                                                                      \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, strm_, __VA_ARGS__);             \
    LB_HIP(hipGetLastError());                                                             \
    if (si_ >= 0) LB_HIP(hipEventRecord(sl.ev1[si_], strm_));                              \
    LB_COUNT_SYNC();                                                                       \
    if (si_ >= 0) {                                                                        \
      LB_COUNT_TAKE(si_);                                                                  \
    }                                                                                      \
  } while (0)
#define LB_STAGE(name, s, kern, grid, block, ...) LB_STAGE_ON(name, sl.st[s], kern, grid, block, __VA_ARGS__)

// A launch without a stage of its own (no timing events, no name in lb_last_stage_times):
// the launch and its error check in one, so no launch goes unchecked.
#define LB_ENQUEUE(strm, kern, grid, block, ...)                                           \
  do {                                                                                     \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, strm, __VA_ARGS__);              \
    LB_HIP(hipGetLastError());                                                             \
  } while (0)
#define LB_LAUNCH(kern, grid, block, ...) LB_ENQUEUE(ctx->stream, kern, grid, block, __VA_ARGS__)

int lp_ensure(lb_ctx* ctx);
int slot_copy(lb_ctx* ctx, Slot& sl, void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t st);

// The latency path (k_lp.hip) for a small call: pubkeys -> per-set inputs -> one
// workgroup per set (set program, the request's product tree, the root's final
// exponentiation).  No merged check: every request is verified on its own, in
// parallel, which is what the reference's verdicts are per request anyway.
int run_lp(lb_ctx* ctx, Slot& sl, uint32_t n_req, uint32_t n_sets, const uint32_t* d_req_off, const uint8_t* d_pks,
           const uint32_t* d_pk_off, const uint32_t* d_pk_idx, const uint8_t* d_msgs, const uint8_t* d_sigs,
           const uint32_t* d_sig_off, const uint8_t* d_seed, uint8_t* d_valid, uint8_t* d_req_err,
           uint8_t* d_set_status, Slab& ws) {
  LB_TRY(lp_ensure(ctx));
  const uint32_t ns = n_sets ? n_sets : 1;
  const LpLayout lay = layout_lp(ns, !d_set_status, ws.fill);
  if (lay.end > ws.cap) {
    ctx->err = "workspace overflow";
    return LB_ERR_OUT_OF_MEMORY;
  }
  ws.fill = lay.end;
  g1j* d_pk = slab_at<g1j>(ws.base, lay.off[LPB_PK]);
  uint8_t* d_pk_st = slab_at<uint8_t>(ws.base, lay.off[LPB_PK_ST]);
  uint32_t* d_in16 = slab_at<uint32_t>(ws.base, lay.off[LPB_IN16]);
  uint32_t* d_fl = slab_at<uint32_t>(ws.base, lay.off[LPB_FL]);
  uint8_t* d_sig_st = d_set_status ? d_set_status : slab_at<uint8_t>(ws.base, lay.off[LPB_SIG_ST]);
  uint32_t* d_setreq = slab_at<uint32_t>(ws.base, lay.off[LPB_SETREQ]);
  uint32_t* d_F = slab_at<uint32_t>(ws.base, lay.off[LPB_F]);
  uint32_t* d_cnt = slab_at<uint32_t>(ws.base, lay.off[LPB_CNT]);
  unsigned long long* d_clk = slab_at<unsigned long long>(ws.base, lay.off[LPB_CLK]);
  if (!n_sets) {  // every request empty: false (otherwise k_lp_prep zeroes the outputs)
    LB_HIP(hipMemsetAsync(d_valid, 0, n_req, sl.st[0]));
    LB_HIP(hipMemsetAsync(d_req_err, 0, n_req, sl.st[0]));
    return LB_OK;
  }
  const PkSource src{d_pks, d_pk_idx, ctx->table.d, ctx->table.n};
  LB_STAGE("pubkeys", 0, k_pubkeys_single, blocks_for(n_sets), TPB, n_sets, src, d_pk_off, d_pk, d_pk_st);
  if (d_pk_off)
    LB_STAGE("pubkeys_agg", 0, k_pubkeys_agg, n_sets < 16384u ? n_sets : 16384u, TPB, n_sets, src, d_pk_off, d_pk,
             d_pk_st);
  LB_STAGE("lp_prep", 0, k_lp_prep, blocks_for(n_sets), TPB, n_sets, d_req_off, n_req, d_msgs, d_sigs, d_sig_off,
           (const g1j*)d_pk, d_seed, d_in16, d_fl, d_sig_st, d_setreq, d_valid, d_req_err, d_cnt,
           (uint32_t)LB_LP_TREE_LEVELS * ns, d_clk);
  LpCall c;
  c.prog_single = ctx->d_lp.d + LB_LP_PROGS[LB_LP_PROG_SET_SINGLE].off;
  c.prog_batch = ctx->d_lp.d + LB_LP_PROGS[LB_LP_PROG_SET_BATCH].off;
  c.prog_mul = ctx->d_lp.d + LB_LP_PROGS[LB_LP_PROG_MUL].off;
  c.prog_final = ctx->d_lp.d + LB_LP_PROGS[LB_LP_PROG_FINAL].off;
  c.req_off = d_req_off;
  c.set_req = d_setreq;
  c.in16 = d_in16;
  c.flags = d_fl;
  c.sig_st = d_sig_st;
  c.pk_st = d_pk_st;
  c.F = d_F;
  c.cnt = d_cnt;
  c.valid = d_valid;
  c.req_err = d_req_err;
  c.n_sets = n_sets;
  c.clk = d_clk;
  LB_STAGE("lp_verify", 0, k_lp_verify, n_sets, LB_LP_TPB, c);
  LB_TRY(slot_copy(ctx, sl, sl.h_clk, d_clk, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, sl.st[0]));
  sl.lp_call = true;
  PipeState& ps = sl.ps;
  ps = PipeState{};
  ps.n_req = n_req;
  ps.n_sets = n_sets;
  ps.d_valid = d_valid;
  return LB_OK;
}

// stream `to` of the slot waits for everything enqueued so far on stream `from`
int stream_wait(lb_ctx* ctx, Slot& sl, int from, int to, int ev) {
  LB_HIP(hipEventRecord(sl.dep[ev], sl.st[from]));
  LB_HIP(hipStreamWaitEvent(sl.st[to], sl.dep[ev], 0));
  return LB_OK;
}

// Tails of a call (after the per-request products F_k): with a merged check,
// the per-request tails run only when d_mflag[0] == 0 (k_lines_S / k_tail skip
// themselves otherwise); without one, every request runs its tail.
int run_tails(lb_ctx* ctx, Slot& sl) {
  const PipeState& p = sl.ps;
  if (p.merged) {
    if (p.msm) {  // the S_k of the per-request tails (skipped when the merged check passed)
      LB_STAGE("scalar_sig", 0, k_scalar_sig, blocks_for(p.n_sets), TPB, p.n_sets, p.d_seed, p.d_sig, p.d_sig_st,
               p.d_rsig, (const uint8_t*)p.d_mflag);
      LB_STAGE("sum_tree", 0, k_sum_tree, p.n_req, TPB, p.n_req, p.d_req_off, (const g2j*)p.d_rsig, p.d_S,
               (const uint8_t*)p.d_mflag);
    }
    if (!p.d_rt_in)
      LB_STAGE("lines_S", 0, k_lines_S, blocks_for(p.n_req), TPB, p.n_req, p.n_pairs, p.n_sets, (const g2a*)p.d_S,
               p.d_lines, (const uint8_t*)p.d_mflag);
    if (p.steps) {
      const uint32_t sp = p.rows.split;
      LB_STAGE("req_horner", 0, k_req_horner, p.n_req * sp, TPB, p.n_req, p.n_sets, p.rows, p.d_req_off, p.d_G,
               (const uint8_t*)p.d_bad, sp > 1 ? p.d_Fparts : p.d_F, (const uint8_t*)p.d_mflag);
      if (sp > 1)
        LB_STAGE("req_horner", 0, k_req_join, p.n_req, TPB, p.n_req, sp, (const fp12*)p.d_Fparts,
                 (const uint8_t*)p.d_bad, p.d_F, (const uint8_t*)p.d_mflag);
    }
    if (p.d_rt_in) {
      LB_ENQUEUE(sl.st[0], k_rtail_prep, (p.n_req * LB_RTAIL_NIN + 255) / 256, 256, p.n_req, (const fp12*)p.d_F,
                 (const g2a*)p.d_S, p.d_rt_in, p.d_rt_fl);
      LB_STAGE("rtail", 0, k_lp_rtail, p.n_req, LB_LP_TPB, ctx->d_lp.d + LB_LP_PROGS[LB_LP_PROG_RTAIL].off, p.n_req,
               (const uint32_t*)p.d_rt_in, (const uint32_t*)p.d_rt_fl, (const uint8_t*)p.d_bad, p.d_valid,
               (const uint8_t*)p.d_mflag);
    } else {
      LB_STAGE("tail", 0, k_tail, p.n_req, TPB, p.n_req, p.n_pairs, p.n_sets, (const uint32_t*)p.d_lines,
               (const fp12*)p.d_F, (const uint8_t*)p.d_bad, p.d_valid, (const uint8_t*)p.d_mflag);
    }
    LB_ENQUEUE(sl.st[0], k_merge_stats, 1, TPB, p.n_req, p.d_req_off, (const uint8_t*)p.d_bad,
               (const uint8_t*)p.d_mflag, p.d_mstats);
    LB_HIP(hipMemcpyAsync(sl.h_stats, p.d_mstats, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, sl.st[0]));
  } else if (p.tail_wave) {
    LB_STAGE("tail", 0, k_tail, p.n_req, TPB, p.n_req, p.n_pairs, p.n_sets, (const uint32_t*)p.d_lines,
             (const fp12*)p.d_F, (const uint8_t*)p.d_bad, p.d_valid, (const uint8_t*)nullptr);
  } else {
    LB_STAGE("final_exp", 0, k_final, blocks_for(p.n_req), TPB, p.n_req, (const fp12*)p.d_F, (const uint8_t*)p.d_bad,
             p.d_valid);
  }
  return LB_OK;
}

static bool any_slot_busy(const lb_ctx* ctx) {
  for (int s = 0; s <= ctx->plan.n_slots; s++)
    if (ctx->slots[s].busy) return true;
  return false;
}

// the GPU is this call's: no other throughput slot busy, the slots lent to the call apart
static bool call_is_lone(const lb_ctx* ctx, const Slot& sl) {
  for (int s = 0; s < ctx->plan.n_slots; s++)
    if (&ctx->slots[s] != &sl && ctx->slots[s].busy && ctx->slots[s].lent_to != &sl) return false;
  return true;
}

static_assert(sizeof(g2j) == SZ_G2J && sizeof(g1j) == SZ_G1J && sizeof(g2a) == SZ_G2A && sizeof(fp12) == SZ_FP12 &&
                  LB_GT_BYTES == SZ_FP12,
              "bls_plan.h lays the workspace out with these record sizes");

// A pipeline call's device pointers: what the caller passed, and the workspace buffers of
// its layout (bls_plan.h PipeBuf, same order; nullptr: the plan has no such buffer).
struct PipeBufs {
  const uint32_t* req_off;
  const uint8_t* pks;
  const uint32_t *pk_off, *pk_idx;
  const uint8_t *msgs, *sigs;
  const uint32_t* sig_off;
  const uint8_t* seed;
  uint8_t *valid, *req_err, *partial;
  g2j *sig, *rsig, *q, *h;
  g1j *pk, *rpk;
  fp12* f;  // per-set Miller values (lane / wave organisations)
  uint32_t* lines;
  uint8_t *single, *pk_st, *sig_st;
  g2a* S;
  fp12 *fS, *F;
  uint32_t *rt_in, *rt_fl;
  uint8_t* bad;
  g2a* Sall;
  fp12* Fall;
  uint8_t* mflag;
  uint32_t* mstats;
  uint32_t *mkeys, *msorted, *mhist;
  g2j *mcsum, *mbsum, *mG;
  uint32_t *rhist, *rgt, *rowoff, *rpos, *rinv, *rmeta, *G;
  fp12* Fparts;
  uint32_t *dec_in, *dec_fl, *dec_out, *dec_ofl;
  uint8_t* dec_pre;
  uint32_t *hf_in, *hf_out, *ll_in, *ll_out;
  fp12 *Pl, *lvA, *lvB;
  uint8_t *lhA, *lhB;
  uint32_t *mt_in, *mt_out, *mb_in0, *mb_in1, *mb_in2;
  fp12* Fx;
  uint32_t* off2;
  fp12* acc_F;
  uint8_t *acc_bad, *acc_err;
  Rows rows;
  hipStream_t ts;  // the merged check's stream: the slot's own, or the shared high-priority one (LB_TAIL_PRIO=1)
};

template <class T>
static T* buf_at(char* base, const PipeLayout& L, PipeBuf b) {
  return L.has(b) ? reinterpret_cast<T*>(base + L.off[b]) : nullptr;
}

static void bind_workspace(PipeBufs& b, char* base, const PipeLayout& L, uint32_t lsplit) {
  b.sig = buf_at<g2j>(base, L, PB_SIG);
  b.rsig = buf_at<g2j>(base, L, PB_RSIG);
  b.q = buf_at<g2j>(base, L, PB_Q);
  b.h = buf_at<g2j>(base, L, PB_H);
  b.pk = buf_at<g1j>(base, L, PB_PK);
  b.rpk = buf_at<g1j>(base, L, PB_RPK);
  b.f = buf_at<fp12>(base, L, PB_F_SETS);
  b.lines = buf_at<uint32_t>(base, L, PB_LINES);
  b.single = buf_at<uint8_t>(base, L, PB_SINGLE);
  b.pk_st = buf_at<uint8_t>(base, L, PB_PK_ST);
  b.sig_st = buf_at<uint8_t>(base, L, PB_SIG_ST);
  b.S = buf_at<g2a>(base, L, PB_S);
  b.fS = buf_at<fp12>(base, L, PB_FS);
  b.F = buf_at<fp12>(base, L, PB_F);
  b.rt_in = buf_at<uint32_t>(base, L, PB_RT_IN);
  b.rt_fl = buf_at<uint32_t>(base, L, PB_RT_FL);
  b.bad = buf_at<uint8_t>(base, L, PB_BAD);
  b.Sall = buf_at<g2a>(base, L, PB_SALL);
  b.Fall = buf_at<fp12>(base, L, PB_FALL);
  b.mflag = buf_at<uint8_t>(base, L, PB_MFLAG);
  b.mstats = buf_at<uint32_t>(base, L, PB_MSTATS);
  b.mkeys = buf_at<uint32_t>(base, L, PB_MKEYS);
  b.msorted = buf_at<uint32_t>(base, L, PB_MSORTED);
  b.mhist = buf_at<uint32_t>(base, L, PB_MHIST);
  b.mcsum = buf_at<g2j>(base, L, PB_MCSUM);
  b.mbsum = buf_at<g2j>(base, L, PB_MBSUM);
  b.mG = buf_at<g2j>(base, L, PB_MG);
  b.rhist = buf_at<uint32_t>(base, L, PB_RHIST);
  b.rgt = buf_at<uint32_t>(base, L, PB_RGT);
  b.rowoff = buf_at<uint32_t>(base, L, PB_ROWOFF);
  b.rpos = buf_at<uint32_t>(base, L, PB_RPOS);
  b.rinv = buf_at<uint32_t>(base, L, PB_RINV);
  b.rmeta = buf_at<uint32_t>(base, L, PB_RMETA);
  b.G = buf_at<uint32_t>(base, L, PB_G);
  b.Fparts = buf_at<fp12>(base, L, PB_FPARTS);
  b.dec_in = buf_at<uint32_t>(base, L, PB_DEC_IN);
  b.dec_fl = buf_at<uint32_t>(base, L, PB_DEC_FL);
  b.dec_out = buf_at<uint32_t>(base, L, PB_DEC_OUT);
  b.dec_ofl = buf_at<uint32_t>(base, L, PB_DEC_OFL);
  b.dec_pre = buf_at<uint8_t>(base, L, PB_DEC_PRE);
  b.hf_in = buf_at<uint32_t>(base, L, PB_HF_IN);
  b.hf_out = buf_at<uint32_t>(base, L, PB_HF_OUT);
  b.ll_in = buf_at<uint32_t>(base, L, PB_LL_IN);
  b.ll_out = buf_at<uint32_t>(base, L, PB_LL_OUT);
  b.Pl = buf_at<fp12>(base, L, PB_PL);
  b.lvA = buf_at<fp12>(base, L, PB_LVA);
  b.lvB = buf_at<fp12>(base, L, PB_LVB);
  b.lhA = buf_at<uint8_t>(base, L, PB_LHA);
  b.lhB = buf_at<uint8_t>(base, L, PB_LHB);
  b.mt_in = buf_at<uint32_t>(base, L, PB_MT_IN);
  b.mt_out = buf_at<uint32_t>(base, L, PB_MT_OUT);
  b.mb_in0 = buf_at<uint32_t>(base, L, PB_MB_IN0);
  b.mb_in1 = buf_at<uint32_t>(base, L, PB_MB_IN1);
  b.mb_in2 = buf_at<uint32_t>(base, L, PB_MB_IN2);
  b.Fx = buf_at<fp12>(base, L, PB_FX);
  b.off2 = buf_at<uint32_t>(base, L, PB_OFF2);
  b.acc_F = buf_at<fp12>(base, L, PB_ACC_F);
  b.acc_bad = buf_at<uint8_t>(base, L, PB_ACC_BAD);
  b.acc_err = buf_at<uint8_t>(base, L, PB_ACC_ERR);
  b.partial = buf_at<uint8_t>(base, L, PB_PARTIAL);
  b.rows = Rows{b.rowoff, b.rinv, b.rpos, b.rmeta, lsplit};
}

// ---- kernel variants by plan field ----------------------------------------------------------
static decltype(&k_lines<1>) lines_kernel(const PipePlan& p) { return p.lines_W == 1 ? k_lines<1> : k_lines<2>; }
static decltype(&k_lines_rows<1>) lines_rows_kernel(const PipePlan& p) {
  return p.lines_W == 1 ? k_lines_rows<1> : k_lines_rows<2>;
}
static decltype(&k_step_acc<0, 1>) step_acc_kernel(const PipePlan& p) {
  if (p.pair_pre) {  // (never with step_M == 2: plan_pipeline)
    if (p.step_M == 1) return k_step_acc<1, 1, true>;
    return p.step_W == 2 ? k_step_acc<0, 2, true> : k_step_acc<0, 1, true>;
  }
  if (p.step_M == 1) return k_step_acc<1, 1>;
  if (p.step_M == 2) return p.step_W == 2 ? k_step_acc<2, 2> : k_step_acc<2, 1>;
  return p.step_W == 2 ? k_step_acc<0, 2> : k_step_acc<0, 1>;
}
static decltype(&k_miller_acc<64>) miller_acc_kernel(const PipePlan& p) {
  return p.acc_lpr == 16 ? k_miller_acc<16> : p.acc_lpr == 32 ? k_miller_acc<32> : k_miller_acc<64>;
}

static const uint32_t* lp_prog(const lb_ctx* ctx, int prog) { return ctx->d_lp.d + LB_LP_PROGS[prog].off; }

// ---- the stages, in the order run_pipeline enqueues them ------------------------------------
// Each tests plan fields only.  Stream 0 carries the call's spine, stream 1 the hash and the lines.

// hash_to_G2 of every message (stream 1): two lanes per message and the finish, the finish as
// round programs, or the whole curve part as one program per set
static int enqueue_hash(lb_ctx* ctx, Slot& sl, const PipePlan& p, const PipeBufs& b) {
  const uint32_t n_sets = p.n_sets;
  if (p.hash == HASH_NONE) return LB_OK;
  if (p.hash == HASH_FULL_LP) {
    LB_STAGE("hash_finish", 1, k_hu_prep, blocks_for(n_sets, 256), 256u, n_sets, b.msgs, b.hf_in);
    LB_STAGE("hash_finish", 1, k_lp_hash, n_sets, LB_LP_NARROW_ROWS * 16u, lp_prog(ctx, LB_LP_PROG_HASH_FULL), n_sets,
             (const uint32_t*)b.hf_in, b.hf_out);
    LB_STAGE("hash_finish", 1, k_hf_finish, blocks_for(n_sets * 6u, 256), 256u, n_sets, (const uint32_t*)b.hf_out, b.h);
    return LB_OK;
  }
  LB_STAGE("hash_half", 1, k_hash_half, blocks_for(2 * n_sets), TPB, n_sets, b.msgs, b.q);
  if (p.hash == HASH_FINISH_LP) {  // clear_cofactor(Q0 + Q1) as round programs, k_lp_hf
    LB_STAGE("hash_finish", 1, k_hf_prep, blocks_for(n_sets * 12u, 256), 256u, n_sets, (const g2j*)b.q, b.hf_in);
    LB_STAGE("hash_finish", 1, k_lp_hf, n_sets, (p.hf_narrow ? LB_LP_NARROW_ROWS : LB_LP_HF_ROWS) * 16u,
             lp_prog(ctx, p.hf_narrow ? LB_LP_PROG_HASH_FINISH_NARROW : LB_LP_PROG_HASH_FINISH), n_sets,
             (const uint32_t*)b.hf_in, b.hf_out);
    LB_STAGE("hash_finish", 1, k_hf_finish, blocks_for(n_sets * 6u, 256), 256u, n_sets, (const uint32_t*)b.hf_out, b.h);
  } else {
    LB_STAGE("hash_finish", 1, k_hash_finish, blocks_for(n_sets), TPB, n_sets, b.q, b.h);
  }
  return LB_OK;
}

// request flags, and for the steps organisation the size-descending order of the requests and
// the row offsets (before stream 1's lines)
static int enqueue_row_order(lb_ctx* ctx, Slot& sl, const PipePlan& p, const PipeBufs& b) {
  LB_STAGE("req_flags", 0, k_req_flags, blocks_for(p.n_req), TPB, p.n_req, b.req_off, b.single);
  if (!p.steps) return LB_OK;
  uint32_t* d_rcur = b.rhist + (p.ns + 1);
  LB_HIP(hipMemsetAsync(b.rhist, 0, 2 * ((size_t)p.ns + 1) * sizeof(uint32_t), sl.st[0]));
  LB_ENQUEUE(sl.st[0], k_rows_hist, blocks_for(p.n_req, 256), 256, p.n_req, b.req_off, b.rhist);
  LB_ENQUEUE(sl.st[0], k_rows_scan, 1, 1024, p.n_sets, (const uint32_t*)b.rhist, b.rgt, b.rowoff, b.rmeta);
  LB_ENQUEUE(sl.st[0], k_rows_pos, blocks_for(p.n_req, 256), 256, p.n_req, b.req_off, (const uint32_t*)b.rgt, d_rcur,
             b.rpos, b.rinv);
  return LB_OK;
}

// PublicKey.fromBytes + aggregate, then r_i pk_i
static int enqueue_pubkeys(lb_ctx* ctx, Slot& sl, const PipePlan& p, const PipeBufs& b) {
  const uint32_t n_sets = p.n_sets;
  if (!n_sets) return LB_OK;
  const PkSource src{b.pks, b.pk_idx, ctx->table.d, ctx->table.n};
  LB_STAGE("pubkeys", 0, k_pubkeys_single, blocks_for(n_sets), TPB, n_sets, src, b.pk_off, b.pk, b.pk_st);
  if (b.pk_off)
    // one wave per set, grid-stride: enough waves that every aggregate of a
    // C4/C5-sized call (thousands of committee sets) gets its own
    LB_STAGE("pubkeys_agg", 0, k_pubkeys_agg, n_sets < 16384u ? n_sets : 16384u, TPB, n_sets, src, b.pk_off, b.pk,
             b.pk_st);
  LB_STAGE("scalar_pk", 0, k_scalar_pk, blocks_for(n_sets), TPB, n_sets, b.seed, (const g1j*)b.pk,
           (const uint8_t*)b.single, b.pk_st, b.rpk);
  return LB_OK;
}

// the lines of (r_i pk_i, H_i) or the per-set Miller values (stream 1)
static int enqueue_lines(lb_ctx* ctx, Slot& sl, const PipePlan& p, const PipeBufs& b) {
  const uint32_t n_sets = p.n_sets, n_pairs = p.n_pairs;
  if (p.lines == LINES_LP) {
    // (a lone mid-size call: each slot's 68 lines as a round program, k_lp_lines)
    LB_STAGE("lines", 1, k_lines_prep, blocks_for(n_sets * 9u, 256), 256u, n_sets, b.rows, b.req_off, (const g1j*)b.rpk,
             (const g2j*)b.h, b.ll_in);
    LB_STAGE("lines", 1, k_lp_lines, n_sets, LB_LP_HF_ROWS * 16u, lp_prog(ctx, LB_LP_PROG_LINES), n_sets,
             (const uint32_t*)b.ll_in, b.ll_out);
    LB_STAGE("lines", 1, k_lines_store, (uint32_t)(((size_t)n_sets * LB_MILLER_LINES * 72 + 255) / 256), 256u, n_sets,
             n_pairs, (const uint32_t*)b.ll_out, b.lines);
  } else if (p.lines == LINES_ROWS) {
    LB_STAGE("lines", 1, lines_rows_kernel(p), blocks_for(n_sets), TPB, n_sets, n_pairs, b.rows, b.req_off,
             (const g1j*)b.rpk, b.h, b.lines);
  } else if (p.lines == LINES_PLAIN) {
    LB_STAGE("lines", 1, lines_kernel(p), blocks_for(n_sets), TPB, n_sets, n_pairs, 0u, (const g1j*)b.rpk,
             (const g2j*)b.h, b.lines);
  }
  if (p.miller_wave)
    LB_STAGE("miller_wave", 1, k_pair_wc, n_sets, TPB, n_sets, n_pairs, (const uint32_t*)b.lines, b.f);
  else if (p.miller_sets)
    LB_STAGE("miller_sets", 1, k_miller_sets, blocks_for(n_sets), TPB, n_sets, (const g1j*)b.rpk, (const g2j*)b.h, b.f);
  return LB_OK;
}

// Signature.fromBytes(validate=true), and r_i sig_i where the MSM does not take their sum
static int enqueue_decode(lb_ctx* ctx, Slot& sl, const PipePlan& p, const PipeBufs& b) {
  const uint32_t n_sets = p.n_sets;
  if (!n_sets) return LB_OK;
  if (p.decode == DECODE_LP) {
    // (a lone mid-size call: the signatures' decode as round programs, k_lp_dec -- its one-lane
    // chain is ~5.7 ms whatever the count below the GPU's width)
    LB_STAGE("decode_sigs", 0, k_sm_dec_prep, blocks_for(n_sets, 256), 256u, n_sets, b.sigs, b.sig_off, b.dec_in,
             b.dec_fl, b.dec_pre);
    LB_STAGE("decode_sigs", 0, k_lp_dec, n_sets, LB_LP_DEC_ROWS * 16u, lp_prog(ctx, LB_LP_PROG_SIG_DECODE), n_sets,
             (const uint32_t*)b.dec_in, (const uint32_t*)b.dec_fl, b.dec_out, b.dec_ofl);
    LB_STAGE("decode_sigs", 0, k_sm_dec_finish, blocks_for(n_sets, 256), 256u, n_sets, (const uint8_t*)b.dec_pre,
             (const uint32_t*)b.dec_in, (const uint32_t*)b.dec_fl, (const uint32_t*)b.dec_out,
             (const uint32_t*)b.dec_ofl, b.sig, b.sig_st, (const uint8_t*)b.single);
  } else if (p.decode == DECODE_PLAIN) {
    LB_STAGE("decode_sigs", 0, k_decode_sigs, blocks_for(n_sets), TPB, n_sets, b.sigs, b.sig_off,
             (const uint8_t*)b.single, b.sig, b.sig_st);
  }
  if (!p.use_msm)
    LB_STAGE("scalar_sig", 0, k_scalar_sig, blocks_for(n_sets), TPB, n_sets, b.seed, (const g2j*)b.sig,
             (const uint8_t*)b.sig_st, b.rsig, (const uint8_t*)nullptr);
  return LB_OK;
}

// request status of the steps organisation (k_miller_acc's side reduction in the pairs organisation)
static int enqueue_req_status(lb_ctx* ctx, Slot& sl, const PipePlan& p, const PipeBufs& b) {
  if (p.steps)
    LB_STAGE("req_status", 0, k_req_status, p.n_req < 4096u ? p.n_req : 4096u, TPB, p.n_req, b.req_off,
             (const uint8_t*)b.sig_st, (const uint8_t*)b.pk_st, b.bad, b.req_err);
  return LB_OK;
}

// S_all = sum r_i sig_i over the good requests' sets: one bucket MSM (k_msm.hip)
static int enqueue_msm(lb_ctx* ctx, Slot& sl, const PipePlan& p, const PipeBufs& b) {
  const uint32_t n_req = p.n_req, n_sets = p.n_sets, n_pairs = p.n_pairs;
  uint32_t* d_off = b.mhist + (LB_MSM_BUCKETS + 1);
  uint32_t* d_coff = d_off + (LB_MSM_BUCKETS + 1);
  uint32_t* d_cur = d_coff + (LB_MSM_BUCKETS + 1);
  LB_HIP(hipMemsetAsync(b.mhist, 0, (LB_MSM_BUCKETS + 1) * sizeof(uint32_t), sl.st[0]));
  LB_STAGE("msm_digits", 0, k_msm_scalars, n_req, TPB, n_req, b.req_off, b.seed, (const uint64_t*)nullptr,
           (const g2j*)b.sig, (const uint8_t*)b.sig_st, (const uint8_t*)b.pk_st, b.mkeys, b.mhist);
  LB_ENQUEUE(sl.st[0], k_msm_scan, 1, 1024, (const uint32_t*)b.mhist, d_off, d_coff, d_cur, p.msm_T);
  LB_ENQUEUE(sl.st[0], k_msm_scatter, blocks_for((uint32_t)p.n_ent, 256), 256, (uint32_t)p.n_ent,
             (const uint32_t*)b.mkeys, (const uint32_t*)d_off, d_cur, b.msorted);
  LB_STAGE("msm_chunks", 0, k_msm_chunks, blocks_for((uint32_t)p.max_chunks), TPB, (uint32_t)p.max_chunks,
           (const uint32_t*)d_off, (const uint32_t*)d_coff, (const uint32_t*)b.msorted, (const g2j*)b.sig, b.mcsum,
           p.msm_T);
  const uint32_t bl = p.msm_wide ? LB_MSM_BLANES : 1u;
  LB_STAGE("msm_buckets", 0, k_msm_buckets, blocks_for(LB_MSM_BUCKETS * bl), TPB, (const uint32_t*)d_coff,
           (const g2j*)b.mcsum, b.mbsum, bl);
  if (p.bits_lp) {
    // (a lone call's bit sums as three levels of round programs, 8:1 each; the last writes the
    // 33 G_p into the merged-check program's input records, so k_mtail_prep skips them)
    LB_STAGE("msm_bits", 0, k_msm_bits_prep, blocks_for(LB_MSM_BITS_INST * LB_MSM_BITS_GROUP * 6u, 256), 256u,
             (const g2j*)b.mbsum, b.mb_in0);
    constexpr uint32_t NI = LB_MSM_BITS_GROUP * 6u;
    LB_STAGE("msm_bits", 0, k_lp_msm_bits, LB_MSM_BITS_INST, LB_LP_TPB, lp_prog(ctx, LB_LP_PROG_MSM_BITS0),
             (uint32_t)LB_MSM_BITS_INST, NI, 6u, (const uint32_t*)b.mb_in0, b.mb_in1);
    LB_STAGE("msm_bits", 0, k_lp_msm_bits, LB_MSM_BITS_INST / 8u, LB_LP_TPB, lp_prog(ctx, LB_LP_PROG_MSM_BITS1),
             (uint32_t)LB_MSM_BITS_INST / 8u, NI, 6u, (const uint32_t*)b.mb_in1, b.mb_in2);
    LB_STAGE("msm_bits", 0, k_lp_msm_bits, LB_MSM_POS, LB_LP_TPB, lp_prog(ctx, LB_LP_PROG_MSM_BITS2),
             (uint32_t)LB_MSM_POS, NI, 6u, (const uint32_t*)b.mb_in2, b.mt_in + (size_t)12 * LB_MTAIL_LEVELS * 16);
  } else if (p.msm_wide) {
    LB_STAGE("msm_bits", 0, k_msm_bits<LB_MSM_BITS_TPB>, LB_MSM_POS, LB_MSM_BITS_TPB, (const g2j*)b.mbsum, b.mG);
  } else {
    LB_STAGE("msm_bits", 0, k_msm_bits<TPB>, LB_MSM_POS, TPB, (const g2j*)b.mbsum, b.mG);
  }
  if (!p.mtail) LB_STAGE("msm_final", 0, k_msm_final, 1u, TPB, (const g2j*)b.mG, b.Sall);
  // (the merged pair's lines, on stream 0 beside stream 1's hash / lines, unless k_miller_acc
  // folds the pair in or the merged-check program computes its Miller value)
  if (!p.fold && !p.mtail)
    LB_STAGE("lines_all", 0, k_lines_S, 1u, TPB, 1u, n_pairs, n_sets + n_req, (const g2a*)b.Sall, b.lines,
             (const uint8_t*)nullptr);
  return LB_OK;
}

// S_k per request from the per-set ladders; then what the tails need of them before the accumulation
static int enqueue_sums(lb_ctx* ctx, Slot& sl, const PipePlan& p, const PipeBufs& b) {
  const uint32_t n_req = p.n_req, n_sets = p.n_sets, n_pairs = p.n_pairs;
  if (p.use_msm) {
    LB_TRY(enqueue_msm(ctx, sl, p, b));
  } else {
    LB_STAGE("sum_tree", 0, k_sum_tree, n_req, TPB, n_req, b.req_off, (const g2j*)b.rsig, b.S, (const uint8_t*)nullptr);
    if (p.steps && p.merged) {  // S_all of the good requests and its lines, ahead of the level products
      LB_STAGE("merge", 0, k_merge, 1u, TPB, n_req, (const g2a*)b.S, (const fp12*)nullptr, (const uint8_t*)b.bad, b.Sall,
               (fp12*)nullptr, (const fp12*)nullptr);
      LB_STAGE("lines_all", 0, k_lines_S, 1u, TPB, 1u, n_pairs, n_sets + n_req, (const g2a*)b.Sall, b.lines,
               (const uint8_t*)nullptr);
    }
  }
  if (p.tail_wave && !p.merged)
    LB_STAGE("lines_S", 0, k_lines_S, blocks_for(n_req), TPB, n_req, n_pairs, n_sets, (const g2a*)b.S, b.lines,
             (const uint8_t*)nullptr);
  else if (!p.tail_wave)
    LB_STAGE("miller_S", 0, k_miller_S, blocks_for(n_req), TPB, n_req, (const g2a*)b.S, b.fS);
  return LB_OK;
}

// steps organisation: step-major lanes, then the level products and their Horner chain (merged)
// or the per-request Horner values
static int enqueue_acc_steps(lb_ctx* ctx, Slot& sl, const PipePlan& p, const PipeBufs& b) {
  const uint32_t n_req = p.n_req, n_sets = p.n_sets, n_pairs = p.n_pairs, lsplit = p.lsplit;
  // (steps + merged: the merged pair's lines come from a one-lane kernel before the
  // accumulation; as an extra workgroup of k_step_acc they measured 4.8 -> 8.2 ms: the
  // 1,025th wave waits for a SIMD of the 1,024 set waves, then runs the 3.4 ms line chain)
  if (p.pair_pre)  // the pairs' line products first, in place, at two waves per SIMD (k_steps.hip)
    LB_STAGE("step_acc", 0, k_line_pairs, blocks_for(n_sets * lsplit * (LB_MILLER_LINES / lsplit / 2u)), TPB, n_sets,
             n_pairs, b.rows, b.req_off, b.lines);
  LB_STAGE("step_acc", 0, step_acc_kernel(p), blocks_for(n_sets * lsplit), TPB, n_sets, n_pairs, b.rows, b.req_off,
           (const uint32_t*)b.lines, b.G);
  if (!p.merged) {
    LB_STAGE("req_horner", 0, k_req_horner, n_req * lsplit, TPB, n_req, n_sets, b.rows, b.req_off, (const uint32_t*)b.G,
             (const uint8_t*)b.bad, lsplit > 1 ? b.Fparts : b.F, (const uint8_t*)nullptr);
    if (lsplit > 1)
      LB_STAGE("req_horner", 0, k_req_join, n_req, TPB, n_req, lsplit, (const fp12*)b.Fparts, (const uint8_t*)b.bad,
               b.F, (const uint8_t*)nullptr);
    return LB_OK;
  }
  // (mtail: the merged pair's Miller value comes from the round program, not as lines)
  const uint32_t s_pair = p.mtail ? 0xffffffffu : n_sets + n_req;
  if (p.level_wc) {
    const dim3 g_part(p.lvl_per / 256u, 63);
    LB_STAGE("level_prod", 0, k_level_part, g_part, 256u, n_req, n_sets, b.rows, b.req_off, (const uint32_t*)b.G,
             (const uint8_t*)b.bad, p.lvl_per, b.lvA, b.lhA);
    uint32_t pin = p.lvl_per;
    fp12 *src = b.lvA, *dst = b.lvB;
    uint8_t *sh = b.lhA, *dh = b.lhB;
    for (;;) {
      const uint32_t pout = (pin + LB_LVL_GROUP - 1) / LB_LVL_GROUP;
      const dim3 g_wc(pout, 63);
      LB_STAGE("level_wc", 0, k_level_wc, g_wc, TPB, pin, (const fp12*)src, (const uint8_t*)sh, pout, dst, dh, n_pairs,
               s_pair, (const uint32_t*)b.lines, pout == 1 ? b.Pl : (fp12*)nullptr);
      if (pout == 1) break;
      pin = pout;
      std::swap(src, dst);
      std::swap(sh, dh);
    }
  } else {
    LB_STAGE("level_prod", 0, k_level_prod, 63u, 256u, n_req, n_sets, n_pairs, s_pair, b.rows, b.req_off,
             (const uint32_t*)b.G, (const uint8_t*)b.bad, (const uint32_t*)b.lines, b.Pl);
  }
  // (mtail: the round program runs the Horner chain over the level products itself, on the
  // Miller loop's squarings of (-g1, S_all): no one-wave k_horner_all)
  if (!p.mtail) LB_STAGE("horner_all", 0, k_horner_all, 1u, TPB, (const fp12*)b.Pl, b.Fall);
  return LB_OK;
}

// pairs organisation: several pairs per lane sharing the Fp12 squarings, the requests whole or
// in halves (k_split_requests / k_join_halves), the merged pair folded in as one more workgroup
static int enqueue_acc_pairs(lb_ctx* ctx, Slot& sl, const PipePlan& p, const PipeBufs& b) {
  const uint32_t n_req = p.n_req, n_pairs = p.n_pairs;
  const fp12* fS_in = p.tail_wave ? nullptr : (const fp12*)b.fS;
  if (p.split)
    LB_ENQUEUE(sl.st[0], k_split_requests, blocks_for(n_req + 1), TPB, n_req, b.req_off, b.off2);
  const uint32_t nr = p.split ? 2 * n_req : n_req;
  const uint32_t rpw = TPB / p.acc_lpr, grid = (nr + rpw - 1) / rpw + (p.fold ? 1u : 0u);
  LB_STAGE("miller_acc", 0, miller_acc_kernel(p), grid, TPB, nr, p.split ? (const uint32_t*)b.off2 : b.req_off, n_pairs,
           (const uint32_t*)b.lines, p.split ? (const fp12*)nullptr : fS_in, (const uint8_t*)b.sig_st,
           (const uint8_t*)b.pk_st, p.split ? b.acc_F : b.F, p.split ? b.acc_bad : b.bad,
           p.split ? b.acc_err : b.req_err, p.split ? 1u : 0u, p.fold ? (const g2a*)b.Sall : (const g2a*)nullptr, b.Fx);
  if (p.split)
    LB_STAGE("join_halves", 0, k_join_halves, blocks_for(n_req), TPB, n_req, b.req_off, (const fp12*)b.acc_F,
             (const uint8_t*)b.acc_bad, (const uint8_t*)b.acc_err, fS_in, b.F, b.bad, b.req_err);
  return LB_OK;
}

// the per-request products F_k (or, steps + merged, the call's level products)
static int enqueue_accumulate(lb_ctx* ctx, Slot& sl, const PipePlan& p, const PipeBufs& b) {
  if (p.steps) return enqueue_acc_steps(ctx, sl, p, b);
  if (p.by_lines) return enqueue_acc_pairs(ctx, sl, p, b);
  LB_STAGE("prod_tree", 0, k_prod_tree, p.n_req, TPB, p.n_req, b.req_off, (const fp12*)b.f,
           p.tail_wave ? (const fp12*)nullptr : (const fp12*)b.fS, (const uint8_t*)b.sig_st, (const uint8_t*)b.pk_st, b.F,
           b.bad, b.req_err);
  return LB_OK;
}

// Merged check: one tail for the whole call; per-request tails only if it fails.  A two-phase
// call stops at the merged Miller product instead.  On b.ts: the slot's stream 0, or with
// LB_TAIL_PRIO=1 a shared high-priority stream (measured slower, off by default).
// *tails: whether the per-request tails follow now (not for a two-phase call that holds its slot)
static int enqueue_merged(lb_ctx* ctx, Slot& sl, const PipePlan& p, const PipeBufs& b, bool* tails) {
  const uint32_t n_req = p.n_req, n_sets = p.n_sets, n_pairs = p.n_pairs;
  const hipStream_t ts = b.ts;
  *tails = true;
  if (ts != sl.st[0]) {
    LB_HIP(hipEventRecord(sl.dep[3], sl.st[0]));
    LB_HIP(hipStreamWaitEvent(ts, sl.dep[3], 0));
  }
  LB_HIP(hipMemsetAsync(b.mflag, 0, 2, ts));
  if (!p.steps) {  // (steps: F_all from the level products and the Horner chain, S_all's lines included)
    LB_STAGE_ON("merge", ts, k_merge, 1u, TPB, n_req, p.use_msm ? (const g2a*)nullptr : (const g2a*)b.S,
                (const fp12*)b.F, (const uint8_t*)b.bad, b.Sall, b.Fall, (const fp12*)b.Fx);
    if (!p.use_msm)  // (with the MSM: folded into k_miller_acc, or stored right after the MSM)
      LB_STAGE_ON("lines_all", ts, k_lines_S, 1u, TPB, 1u, n_pairs, n_sets + n_req, (const g2a*)b.Sall, b.lines,
                  (const uint8_t*)nullptr);
  }
  const uint32_t* merged_lines = (p.fold || p.steps) ? nullptr : (const uint32_t*)b.lines;
  const uint32_t mt_tpb = p.mt_wide ? LB_LP_MTAIL_ROWS * 16u : (uint32_t)LB_LP_TPB;
  if (p.mtail) {
    LB_ENQUEUE(ts, k_mtail_prep, 1, 256, (const fp12*)b.Pl, p.bits_lp ? (const g2j*)nullptr : (const g2j*)b.mG, b.mt_in);
    if (p.partial) {  // F_all * Miller(-g1, S_all) back into Fall, encoded by k_partial below
      LB_STAGE_ON("mtail", ts, k_lp_mtail, 1u, mt_tpb,
                  lp_prog(ctx, p.mt_wide ? LB_LP_PROG_MTAIL_PARTIAL_WIDE : LB_LP_PROG_MTAIL_PARTIAL),
                  (const uint32_t*)b.mt_in, (uint8_t*)nullptr, b.mt_out);
      LB_ENQUEUE(ts, k_records_to_fp12, 1, 64, (const uint32_t*)b.mt_out, b.Fall);
    }
  }
  if (p.partial) {
    // two-phase call: the merged Miller product goes to the host, which
    // combines it with the other GPUs' partials; the tails wait for its verdict
    LB_STAGE_ON("partial", ts, k_partial, 1u, TPB, n_pairs, n_sets + n_req, merged_lines, (const fp12*)b.Fall,
                b.partial);
    LB_HIP(hipMemcpyAsync(sl.h_partial, b.partial, LB_GT_BYTES, hipMemcpyDeviceToHost, ts));
    LB_HIP(hipEventRecord(sl.partial_ev, ts));
  } else if (p.mtail) {
    LB_STAGE_ON("mtail", ts, k_lp_mtail, 1u, mt_tpb,
                lp_prog(ctx, p.mt_wide ? LB_LP_PROG_MTAIL_CHECK_WIDE : LB_LP_PROG_MTAIL_CHECK), (const uint32_t*)b.mt_in,
                b.mflag, (uint32_t*)nullptr);
  } else {
    LB_STAGE_ON("tail_all", ts, k_tail, 1u, TPB, 1u, n_pairs, n_sets + n_req, merged_lines, (const fp12*)b.Fall,
                (const uint8_t*)(b.mflag + 1), b.mflag, (const uint8_t*)nullptr);
  }
  if (ts != sl.st[0]) {
    LB_HIP(hipEventRecord(sl.dep[4], ts));
    LB_HIP(hipStreamWaitEvent(sl.st[0], sl.dep[4], 0));
  }
  if (p.partial) {
    if (p.tp_release) {
      // the call completes on its own as if the combined check passed (every request not
      // already false valid: no per-request work) and frees its slot at once; a failed
      // combined check re-verifies the shard as a one-phase call (lb_verify_requests_finish)
      LB_HIP(hipMemsetAsync(b.mflag, 1, 1, sl.st[0]));
    } else {
      sl.partial_pending = true;
      *tails = false;
    }
  }
  return LB_OK;
}

// what the tails need of a call (run_tails, now or after lb_verify_requests_finish)
static void fill_state(PipeState& ps, const PipePlan& p, const PipeBufs& b) {
  ps.n_req = p.n_req;
  ps.n_sets = p.n_sets;
  ps.n_pairs = p.n_pairs;
  ps.merged = p.merged;
  ps.tail_wave = p.tail_wave;
  ps.msm = p.use_msm;
  ps.d_seed = b.seed;
  ps.d_sig = b.sig;
  ps.d_sig_st = b.sig_st;
  ps.d_rsig = b.rsig;
  ps.d_req_off = b.req_off;
  ps.d_lines = b.lines;
  ps.d_S = b.S;
  ps.d_F = b.F;
  ps.d_rt_in = b.rt_in;
  ps.d_rt_fl = b.rt_fl;
  ps.d_bad = b.bad;
  ps.d_valid = b.valid;
  ps.d_mflag = b.mflag;
  ps.d_mstats = b.mstats;
  ps.steps = p.steps;
  ps.rows = b.rows;
  ps.d_G = b.G;
  ps.d_Fparts = b.Fparts;
}

// Core pipeline on device-resident inputs (all pointers are device pointers): plan the call
// (bls_plan.h), lay its workspace out, check the slab once, then enqueue the stages as a
// two-stream DAG inside the slot:
//   0: flags, row order -> pubkeys -> r_i pk_i -> [ev 1] -> decode sigs -> request status ->
//      S_all (bucket MSM) or S_k (ladders + tree) -> [wait 1] -> accumulation of the stored
//      lines (step-major lanes, level products) -> merged check -> per-request tails
//   1: hash_to_G2 -> [wait ev 1] -> lines of (r_i pk_i, H_i)
// d_sig_pre / d_sst_pre: signatures already decoded and validated (same-message
// phase 2): no decode, d_sigs / d_sig_off unused
int run_pipeline(lb_ctx* ctx, Slot& sl, uint32_t n_req, uint32_t n_sets, const uint32_t* d_req_off,
                 const uint8_t* d_pks, const uint32_t* d_pk_off, const uint32_t* d_pk_idx, const uint8_t* d_msgs, const uint8_t* d_sigs,
                 const uint32_t* d_sig_off, const uint8_t* d_seed, uint8_t* d_valid, uint8_t* d_req_err,
                 uint8_t* d_set_status, Slab& ws, bool partial = false, const g2j* d_sig_pre = nullptr,
                 const uint8_t* d_sst_pre = nullptr) {
  PipeShape shape;
  shape.n_req = n_req;
  shape.n_sets = n_sets;
  shape.lone = call_is_lone(ctx, sl);
  shape.partial = partial;
  shape.presigned = d_sig_pre != nullptr;
  shape.prio_slot = &sl == &ctx->prio();
  const PipePlan plan = plan_pipeline(ctx->cfg, shape);
  sl.h_stats[0] = sl.h_stats[1] = 0;
  if (plan.latency_path)
    return run_lp(ctx, sl, n_req, n_sets, d_req_off, d_pks, d_pk_off, d_pk_idx, d_msgs, d_sigs, d_sig_off, d_seed,
                  d_valid, d_req_err, d_set_status, ws);
  const PipeLayout lay = layout_pipeline(plan, ws.fill);
  if (ws.fill + lay.bytes > ws.cap) {  // (the one capacity check: nothing is enqueued yet)
    ctx->err = "workspace overflow";
    return LB_ERR_OUT_OF_MEMORY;
  }
  if (plan.needs_lp) LB_TRY(lp_ensure(ctx));
  PipeBufs b{};
  b.req_off = d_req_off;
  b.pks = d_pks;
  b.pk_off = d_pk_off;
  b.pk_idx = d_pk_idx;
  b.msgs = d_msgs;
  b.sigs = d_sigs;
  b.sig_off = d_sig_off;
  b.seed = d_seed;
  b.valid = d_valid;
  b.req_err = d_req_err;
  bind_workspace(b, ws.base, lay, plan.lsplit);
  ws.fill += lay.bytes;
  if (d_sig_pre) b.sig = const_cast<g2j*>(d_sig_pre);
  if (d_sst_pre)
    b.sig_st = const_cast<uint8_t*>(d_sst_pre);
  else if (d_set_status)
    b.sig_st = d_set_status;
  b.ts = plan.merged && ctx->tail_stream ? ctx->tail_stream : sl.st[0];

  LB_TRY(stream_wait(ctx, sl, 0, 1, 0));
  LB_TRY(enqueue_hash(ctx, sl, plan, b));
  LB_TRY(enqueue_row_order(ctx, sl, plan, b));
  LB_TRY(enqueue_pubkeys(ctx, sl, plan, b));
  LB_TRY(stream_wait(ctx, sl, 0, 1, 1));
  LB_TRY(enqueue_lines(ctx, sl, plan, b));
  LB_TRY(enqueue_decode(ctx, sl, plan, b));
  LB_TRY(enqueue_req_status(ctx, sl, plan, b));
  LB_TRY(enqueue_sums(ctx, sl, plan, b));
  LB_TRY(stream_wait(ctx, sl, 1, 0, 2));
  LB_TRY(enqueue_accumulate(ctx, sl, plan, b));
  fill_state(sl.ps, plan, b);
  if (plan.merged) {
    bool tails = true;
    LB_TRY(enqueue_merged(ctx, sl, plan, b, &tails));
    if (!tails) return LB_OK;
  }
  return run_tails(ctx, sl);
}

// The workspace a call of at most n_req requests and n_sets sets can take, whichever path and
// switches it runs with (a slab is sized before its call's lone / partial state is known, and
// for later calls: the same-message phase 2, the priority slot).  + 255: the first buffer's
// alignment when the slab's fill at the call is not a multiple of 256.
size_t pipeline_ws_bytes(const lb_ctx* ctx, uint32_t n_req, uint32_t n_sets) {
  return layout_pipeline(plan_upper(ctx->cfg, n_req, n_sets)).bytes + 255;
}

int validate_batch(lb_ctx* ctx, const lb_request_batch* b) {
  if (!b || !b->request_offsets || !b->messages || !b->signatures || !b->sig_offsets || !b->seed ||
      (b->n_sets && !b->pubkeys && !b->pubkey_indices)) {
    ctx->err = "null pointer in lb_request_batch";
    return LB_ERR_INVALID_ARGUMENT;
  }
  return LB_OK;
}

// A keys call's batch (lb_verify_requests_keys*): the sets' keys come from `ks` alone
int validate_keys_batch(lb_ctx* ctx, const lb_request_batch* b, const lb_key_source* ks) {
  if (!b || !ks || !b->request_offsets || !b->messages || !b->signatures || !b->sig_offsets || !b->seed ||
      (b->n_sets && !ks->sets) || (ks->n_pool && !ks->key_pool) || (ks->n_bits_bytes && !ks->bits)) {
    ctx->err = "null pointer in lb_request_batch / lb_key_source";
    return LB_ERR_INVALID_ARGUMENT;
  }
  if (b->pubkeys || b->pk_offsets || b->pubkey_indices) {
    ctx->err = "a keys call's batch has pubkeys, pk_offsets and pubkey_indices NULL";
    return LB_ERR_INVALID_ARGUMENT;
  }
  return LB_OK;
}
int validate_host_batch(lb_ctx* ctx, const lb_request_batch* b, const lb_key_source* ks) {
  return ks ? validate_keys_batch(ctx, b, ks) : validate_batch(ctx, b);
}

// A host <-> device copy of a call on slot sl: on the priority slot a kernel (k_copy_bytes,
// LB_PRIO_KCOPY=0: hipMemcpyAsync), never queued on an SDMA engine behind the throughput
// calls' staging; elsewhere hipMemcpyAsync.  Host buffers are pinned (hipHostMalloc).
int slot_copy(lb_ctx* ctx, Slot& sl, void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t st) {
  if (!n) return LB_OK;
  if (ctx->ccfg.prio_kcopy && &sl == &ctx->prio() && n < (1u << 30)) {
    const size_t blocks = (n / 16 + 255) / 256;
    LB_ENQUEUE(st, k_copy_bytes, blocks < 1 ? 1 : blocks > 512 ? 512 : (unsigned)blocks, 256, (const uint8_t*)src,
               (uint8_t*)dst, (uint32_t)n);
    return LB_OK;
  }
  LB_HIP(hipMemcpyAsync(dst, src, n, kind, st));
  return LB_OK;
}

// Copy a host-buffer call's verdicts from the device into its pinned staging
// (enqueued after the tails; the caller's buffers are filled in finish_slot).
int enqueue_host_out(lb_ctx* ctx, Slot& sl) {
  if (!sl.out_valid) return LB_OK;
  LB_TRY(slot_copy(ctx, sl, sl.hv_valid, sl.dv_valid, sl.out_nr, hipMemcpyDeviceToHost, sl.st[0]));
  LB_TRY(slot_copy(ctx, sl, sl.hv_err, sl.dv_err, sl.out_nr, hipMemcpyDeviceToHost, sl.st[0]));
  if (sl.out_ns) LB_TRY(slot_copy(ctx, sl, sl.hv_sst, sl.dv_sst, sl.out_ns, hipMemcpyDeviceToHost, sl.st[0]));
  return LB_OK;
}

int end_call(lb_ctx* ctx, Slot& sl) {
  LB_TRY(enqueue_host_out(ctx, sl));
  LB_HIP(hipEventRecord(sl.wall1, sl.st[0]));
  LB_HIP(hipEventRecord(sl.done, sl.st[0]));
  return LB_OK;
}

// Second phase of a two-phase call: the host's combined verdict (merged_ok)
// decides whether the per-request tails run (k_lines_S / k_tail skip
// themselves when d_mflag[0] != 0).
int finish_partial(lb_ctx* ctx, Slot& sl, bool merged_ok) {
  if (!sl.partial_pending) return LB_OK;
  sl.partial_pending = false;
  if (sl.ps.n_req) {  // (an empty call has no tails)
    LB_HIP(hipMemsetAsync(sl.ps.d_mflag, merged_ok ? 1 : 0, 1, sl.st[0]));
    LB_TRY(run_tails(ctx, sl));
  }
  return end_call(ctx, sl);
}

// Wait for a slot's outstanding call and publish its stage times, stats and
// (host-buffer calls) verdicts.  A two-phase call whose host verdict never came
// runs its per-request tails (merged_ok = 0: every verdict computed alone).
int sm_advance(lb_ctx* ctx, Slot& sl, bool block);
int sm_pump(lb_ctx* ctx);

void release_borrowed(Slot& sl) {  // hand a borrowed stream back
  if (!sl.borrowed) return;
  sl.borrowed->busy = false;
  sl.borrowed->lent_to = nullptr;
  sl.st[1] = sl.st[0];
  sl.borrowed = nullptr;
}

int finish_slot(lb_ctx* ctx, Slot& sl) {
  if (sl.lent_to) return finish_slot(ctx, *sl.lent_to);  // releases this slot
  if (!sl.busy) {
    release_borrowed(sl);  // (a submission that failed after borrowing)
    return LB_OK;
  }
  LB_TRY(finish_partial(ctx, sl, false));
  while (sl.sm.active && sm_advance(ctx, sl, true) == LB_OK) {
  }  // same-message: phases 1 and 2
  if (sl.sm.err) {  // its phase 2 failed to launch (here or in another call's sm_pump)
    const int rc = sl.sm.err;
    ctx->err = sl.sm.err_msg;
    sl.sm.err = 0;
    for (int i = 0; i < 2; i++) (void)hipStreamSynchronize(sl.st[i]);
    release_borrowed(sl);
    sl.busy = false;
    return rc;
  }
  LB_HIP(hipEventSynchronize(sl.done));
  ctx->n_stages = sl.n_stages;
  for (int i = 0; i < sl.n_stages; i++) {
    float ms = 0.f;
    LB_HIP(hipEventElapsedTime(&ms, sl.ev0[i], sl.ev1[i]));
    ctx->stage_ms[i] = ms;
    ctx->stage_name[i] = sl.stage_name[i];
    ctx->stage_ops[i] = sl.stage_ops[i];
  }
  LB_HIP(hipEventElapsedTime(&ctx->wall_ms, sl.wall0, sl.wall1));
  ctx->batch_retries = sl.h_stats[0];
  ctx->batch_sigs_success = sl.h_stats[1];
  if (sl.lp_call)
    for (int i = 0; i < 4; i++) ctx->lp_clk[i] = sl.h_clk[i];
  {  // a released two-phase call: its partial outlives the slot
    TwoPhaseRec& r = ctx->tp[sl.ticket % lb_ctx::kTwoPhaseRing];
    if (sl.ticket && r.ticket == sl.ticket && !r.have_partial) {
      memcpy(r.partial, sl.h_partial, LB_GT_BYTES);
      r.have_partial = true;
    }
  }
  TicketStats& ts = ctx->tstats[sl.ticket % lb_ctx::kTicketRing];
  ts.ticket = sl.ticket;
  ts.batch_retries = sl.h_stats[0];
  ts.batch_sigs_success = sl.h_stats[1];
  ts.wall_ms = ctx->wall_ms;
  if (sl.out_valid) {
    memcpy(sl.out_valid, sl.hv_valid, sl.out_nr);
    memcpy(sl.out_err, sl.hv_err, sl.out_nr);
    if (sl.out_sst && sl.out_ns) memcpy(sl.out_sst, sl.hv_sst, sl.out_ns);
    sl.out_valid = sl.out_err = sl.out_sst = nullptr;
  }
  release_borrowed(sl);
  sl.busy = false;
  return LB_OK;
}

// An async call on slot `sl` (single stream, just retired) while no other call is
// in flight: the lowest latency is the two-stream DAG (hash_to_G2 + lines beside
// the signature / MSM branch), so it borrows an idle slot's stream; the next call
// that wants that slot waits for this one first (finish_slot).
void borrow_idle_stream(lb_ctx* ctx, Slot& sl) {
  if (!ctx->ccfg.dag || sl.st[1] != sl.st[0] || sl.borrowed || &sl == &ctx->prio()) return;
  Slot* idle = nullptr;
  for (int s = 0; s < ctx->plan.n_slots; s++) {
    Slot& o = ctx->slots[s];
    if (&o == &sl) continue;
    if (o.busy || o.partial_pending) return;  // not alone on the GPU
    if (!idle && o.st[0] != sl.st[0]) idle = &o;
  }
  if (!idle) return;
  sl.st[1] = idle->st[0];
  sl.borrowed = idle;
  idle->busy = true;
  idle->ticket = 0;
  idle->lent_to = &sl;
}

int begin_call(lb_ctx* ctx, Slot& sl) {
  ctx->last_call_streams = sl.st[1] != sl.st[0] ? 2 : 1;
  sl.lp_call = false;
  sl.n_stages = 0;
  sl.partial_pending = false;
  sl.out_valid = sl.out_err = sl.out_sst = nullptr;
  LB_HIP(hipEventRecord(sl.wall0, sl.st[0]));
  return LB_OK;
}
// Mark the slot busy under a new ticket; a complete call also records its end
// (a two-phase call records it in finish_partial).
int end_call_async(lb_ctx* ctx, Slot& sl) {
  if (!sl.partial_pending) LB_TRY(end_call(ctx, sl));
  sl.busy = true;
  sl.ticket = ctx->next_ticket++;
  if (sl.partial_pending) {
    ctx->two_phase[ctx->two_phase_pos] = sl.ticket;
    ctx->two_phase_pos = (ctx->two_phase_pos + 1) % lb_ctx::kTwoPhaseRing;
  }
  return LB_OK;
}

Slot* slot_of_ticket(lb_ctx* ctx, uint64_t ticket) {
  for (int s = 0; s <= ctx->plan.n_slots; s++)
    if (ctx->slots[s].busy && ctx->slots[s].ticket == ticket) return &ctx->slots[s];
  return nullptr;
}

// Synchronous verify calls run on slot 0 as the two-stream DAG.  When slot 0
// owns a single stream (the default four single-stream slots), the call
// borrows slot 1's stream (after slot 1's call in flight completes) and the
// guard hands it back when the call returns (the call is complete by then).
struct BorrowGuard {
  lb_ctx* ctx;
  bool active = false;
  ~BorrowGuard() {
    if (active) {
      ctx->slots[0].guard_st = nullptr;
      ctx->slots[0].st[1] = ctx->slots[0].st[0];
    }
  }
};
int borrow_second_stream(lb_ctx* ctx, BorrowGuard& g) {
  Slot& s0 = ctx->slots[0];
  if (ctx->ccfg.dag && ctx->plan.streams_per_slot[0] == 1 && ctx->plan.n_slots >= 2) {
    LB_TRY(finish_slot(ctx, ctx->slots[1]));
    s0.st[1] = s0.guard_st = ctx->slots[1].st[0];
    g.active = true;
  }
  return LB_OK;
}

// Idle slot 0 for the synchronous helper entry points.
int helper_slot(lb_ctx* ctx) {
  for (int i = 0; i <= ctx->plan.n_slots; i++) LB_TRY(finish_slot(ctx, ctx->slots[i]));
  return LB_OK;
}

// latency path: upload the round programs once (2.6 MB)
int lp_ensure(lb_ctx* ctx) {
  if (ctx->d_lp.d) return LB_OK;
  LB_TRY(ctx->d_lp.reserve(ctx, LB_LP_BLOB_WORDS, 0));
  LB_HIP(hipMemcpy(ctx->d_lp.d, lb_lp_blob, (size_t)LB_LP_BLOB_WORDS * 4, hipMemcpyHostToDevice));
  return LB_OK;
}

}  // namespace

// ============================================================================
// C ABI
// ============================================================================
extern "C" {

int lb_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

static std::string g_create_err = "null context";

// The device as plan_context needs it -- the largest private segment of the kernels a queue
// may run, and the CU count -- and the scratch one hardware queue reserves for them
// (queue_scratch_bytes, bls_ctx_plan.h).
size_t scratch_per_queue(int device, DeviceFacts* out_facts) {
  const void* kernels[] = {(const void*)k_miller_acc<16>, (const void*)k_miller_acc<32>,
                           (const void*)k_miller_acc<64>, (const void*)k_step_acc<0, 1>,
                           (const void*)k_step_acc<0, 2>, (const void*)k_step_acc<1, 1>, (const void*)k_step_acc<2, 1>, (const void*)k_step_acc<2, 2>,
                           (const void*)k_step_acc<0, 1, true>, (const void*)k_step_acc<0, 2, true>,
                           (const void*)k_step_acc<1, 1, true>, (const void*)k_line_pairs, (const void*)k_lines<1>,
                           (const void*)k_lines<2>, (const void*)k_lines_rows<1>, (const void*)k_lines_rows<2>,
                           (const void*)k_pair_wc, (const void*)k_miller_sets,
                           (const void*)k_hash_half, (const void*)k_hash_finish, (const void*)k_final,
                           (const void*)k_tail, (const void*)k_req_horner, (const void*)k_req_join, (const void*)k_lp_verify,
                           (const void*)k_lp_mtail, (const void*)k_lp_final_lane, (const void*)k_gt_prod,
                           (const void*)k_lp_rtail, (const void*)k_lp_msm_bits, (const void*)k_lp_dec, (const void*)k_lp_hf, (const void*)k_lp_hash, (const void*)k_lp_lines, (const void*)k_level_prod, (const void*)k_level_part,
                           (const void*)k_level_wc,
                           (const void*)k_msm_buckets, (const void*)k_msm_bits<TPB>, (const void*)k_msm_bits<LB_MSM_BITS_TPB>,
                           (const void*)k_decode_sigs,
                           (const void*)k_scalar_pk, (const void*)k_sm_rand_pk, (const void*)k_sm_rand_sig,
                           // (the KZG kernels stay below the pipeline's largest: build.py check_kzg_scratch)
                           (const void*)k_kzg_hash, (const void*)k_kzg_eval, (const void*)k_kzg_decode,
                           (const void*)k_kzg_rho, (const void*)k_kzg_ladder, (const void*)k_kzg_miller,
                           (const void*)k_kzg_final,
                           (const void*)k_kzg_setup_g1, (const void*)k_kzg_check_com, (const void*)k_kzg_quotient,
                           (const void*)k_kzg_msm_digits, (const void*)k_kzg_msm_chunks, (const void*)k_kzg_msm_buckets,
                           (const void*)k_kzg_msm_bits, (const void*)k_kzg_msm_final};
  size_t lane = 0;
  for (const void* k : kernels) {
    hipFuncAttributes a{};
    if (hipFuncGetAttributes(&a, k) == hipSuccess && a.localSizeBytes > lane) lane = a.localSizeBytes;
  }
  DeviceFacts f;
  f.lane_bytes = (uint32_t)lane;
  if (hipDeviceGetAttribute(&f.cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) f.cus = 0;
  if (out_facts) *out_facts = f;
  return queue_scratch_bytes(f);
}

// The streams of every live context of this process, by kind (QueueTally, bls_ctx_plan.h).
static std::mutex g_q_mu;
static QueueTally g_q;

static const char* env_lookup(const char* name) { return getenv(name); }

// Facts, plan, resources: the switches and the device, every decision (plan_context: no HIP
// object exists when it refuses), then exactly the streams the plan priced.
static int create_ctx(int device, lb_ctx** out_ctx, bool lane) {
  if (!out_ctx) return LB_ERR_INVALID_ARGUMENT;
  *out_ctx = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0 || device < 0 || device >= n) return LB_ERR_NO_DEVICE;
  bool ok = hipSetDevice(device) == hipSuccess;
  CtxConfig ccfg;
  ctx_config_from_env(ccfg, env_lookup);
  DeviceFacts dev;
  (void)scratch_per_queue(device, &dev);
  CtxPlan plan;
  {
    std::lock_guard<std::mutex> g(g_q_mu);
    plan = plan_context(ccfg, dev, lane, g_q);
    if (plan.err) {
      g_create_err = plan.msg;
      return plan.err;
    }
    g_q.plain += plan.q_plain;
    g_q.high += plan.q_high;
    g_q.masked += plan.q_masked;
  }
  lb_ctx* ctx = new lb_ctx();
  ctx->device = device;
  ctx->ccfg = ccfg;
  ctx->plan = plan;
  config_from_env(ctx->cfg, env_lookup);
  ctx->sm_mode = ccfg.sm_randomized ? LB_SM_RANDOMIZED : LB_SM_PLAIN;
  int prio_least = 0, prio_greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) prio_greatest = 0;
  for (int s = 0; ok && s <= plan.n_slots; s++) {
    Slot& sl = ctx->slots[s];
    for (int i = 0; i < 2; i++) {
      const StreamPlan& e = plan.st[s][i];
      if (e.mask == ST_ALIAS0) sl.st_mask[i] = sl.st_mask[0];
      if (ok && e.mask == ST_OWN)
        ok = hipExtStreamCreateWithCUMask(&sl.st_mask[i], (uint32_t)plan.cu_mask.size(), plan.cu_mask.data()) == hipSuccess;
      if (e.full == ST_ALIAS0) sl.st_full[i] = sl.st_full[0];
      if (ok && e.full == ST_OWN) ok = hipStreamCreateWithFlags(&sl.st_full[i], hipStreamNonBlocking) == hipSuccess;
      if (ok && e.full == ST_HIGH)
        ok = hipStreamCreateWithPriority(&sl.st_full[i], hipStreamNonBlocking, prio_greatest) == hipSuccess;
      sl.st[i] = e.starts_masked() ? sl.st_mask[i] : sl.st_full[i];
    }
    for (int i = 0; ok && i < 8; i++) ok = hipEventCreateWithFlags(&sl.dep[i], hipEventDisableTiming) == hipSuccess;
    for (int i = 0; ok && i < Slot::kMaxStages; i++)
      ok = hipEventCreate(&sl.ev0[i]) == hipSuccess && hipEventCreate(&sl.ev1[i]) == hipSuccess;
    ok = ok && hipEventCreate(&sl.wall0) == hipSuccess && hipEventCreate(&sl.wall1) == hipSuccess &&
         hipEventCreateWithFlags(&sl.done, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&sl.partial_ev, hipEventDisableTiming) == hipSuccess &&
         hipHostMalloc(&sl.h_stats, 4 * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess &&
         hipHostMalloc(&sl.h_partial, LB_GT_BYTES, hipHostMallocDefault) == hipSuccess &&
         hipHostMalloc(&sl.h_clk, 4 * sizeof(unsigned long long), hipHostMallocDefault) == hipSuccess;
    if (ok) sl.h_stats[0] = sl.h_stats[1] = 0;
  }
  ctx->stream = ctx->slots[0].st[0];
  for (hipEvent_t& e : ctx->helper_ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  // the host combine's one-wave final exponentiation must not queue behind the
  // calls in flight (their 1-wave/SIMD kernels fill every SIMD): highest priority
  ok = ok && hipStreamCreateWithPriority(&ctx->aux_stream, hipStreamNonBlocking, prio_greatest) == hipSuccess;
  if (plan.tail_stream)
    ok = ok && hipStreamCreateWithPriority(&ctx->tail_stream, hipStreamNonBlocking, prio_greatest) == hipSuccess;
  // the latency path's round programs (2.6 MB) are uploaded here, before any call is in
  // flight: a synchronous copy on the first latency-path call would wait for the
  // throughput calls already running on blocking (CU-masked) streams
  if (ok && (ctx->cfg.lp_max_sets || ctx->cfg.mtail_lp || ctx->ccfg.gt_lp || ctx->cfg.rtail_lp) && lp_ensure(ctx) != LB_OK)
    ok = false;
  // the priority slot's staging and workspace sized here for a latency-path call of
  // lp_max_sets sets (16 keys each by bytes): growing them later frees the old buffers,
  // and hipFree / hipHostFree synchronize the device -- the call would wait for every
  // throughput call in flight (the node leg's first 128-set priority job under load took
  // 0.9-1.5 s, profiles/r05/node_q/)
  if (ok && ctx->cfg.lp_max_sets) {
    Slot& pl = ctx->slots[ctx->plan.n_slots];
    const size_t ns = ctx->cfg.lp_max_sets;  // (16 keys a set, uncompressed signatures, every set a request)
    const HostCallShape shape{ns, ns, 16 * ns, 192 * ns, 0, true, false};
    const size_t io = layout_host_call(shape).end;
    ok = ensure_pin(ctx, pl, io) == LB_OK &&
         ensure_ws(ctx, pl, io + pipeline_ws_bytes(ctx, (uint32_t)ns, (uint32_t)ns)) == LB_OK;
  }
  if (!ok) {
    lb_destroy(ctx);
    return LB_ERR_DEVICE;
  }
  *out_ctx = ctx;
  return LB_OK;
}

int lb_create(int device, lb_ctx** out_ctx) { return create_ctx(device, out_ctx, false); }

int lb_create_lane(int device, lb_ctx** out_ctx) { return create_ctx(device, out_ctx, true); }

int lb_mark_priority(lb_ctx* ctx) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  ctx->last_prio_ns.store(std::chrono::duration_cast<std::chrono::nanoseconds>(
                              std::chrono::steady_clock::now().time_since_epoch()).count(),
                          std::memory_order_relaxed);
  return LB_OK;
}

int lb_destroy(lb_ctx* ctx) {
  if (!ctx) return LB_OK;
  (void)hipSetDevice(ctx->device);
  for (int s = 0; s <= ctx->plan.n_slots; s++) {
    Slot& sl = ctx->slots[s];
    // the streams the plan made this slot's own (a failed creation left the later ones null)
    hipStream_t own[4];
    int n_own = 0;
    for (int i = 0; i < 2; i++) {
      if (owned(ctx->plan.st[s][i].full) && sl.st_full[i]) own[n_own++] = sl.st_full[i];
      if (owned(ctx->plan.st[s][i].mask) && sl.st_mask[i]) own[n_own++] = sl.st_mask[i];
    }
    for (int i = 0; i < n_own; i++) (void)hipStreamSynchronize(own[i]);
    if (sl.d_ws) (void)hipFree(sl.d_ws);
    if (sl.h_pin) (void)hipHostFree(sl.h_pin);
    for (int i = 0; i < 8; i++)
      if (sl.dep[i]) (void)hipEventDestroy(sl.dep[i]);
    for (int i = 0; i < Slot::kMaxStages; i++) {
      if (sl.ev0[i]) (void)hipEventDestroy(sl.ev0[i]);
      if (sl.ev1[i]) (void)hipEventDestroy(sl.ev1[i]);
    }
    if (sl.wall0) (void)hipEventDestroy(sl.wall0);
    if (sl.wall1) (void)hipEventDestroy(sl.wall1);
    if (sl.done) (void)hipEventDestroy(sl.done);
    if (sl.partial_ev) (void)hipEventDestroy(sl.partial_ev);
    if (sl.h_stats) (void)hipHostFree(sl.h_stats);
    if (sl.h_partial) (void)hipHostFree(sl.h_partial);
    if (sl.h_clk) (void)hipHostFree(sl.h_clk);
    for (int i = 0; i < n_own; i++) (void)hipStreamDestroy(own[i]);
  }
  for (hipEvent_t e : ctx->helper_ev)
    if (e) (void)hipEventDestroy(e);
  if (ctx->aux_stream) {
    (void)hipStreamSynchronize(ctx->aux_stream);
    (void)hipStreamDestroy(ctx->aux_stream);
  }
  if (ctx->tail_stream) {
    (void)hipStreamSynchronize(ctx->tail_stream);
    (void)hipStreamDestroy(ctx->tail_stream);
  }
  if (ctx->d_aux) (void)hipFree(ctx->d_aux);
  if (ctx->h_aux) (void)hipHostFree(ctx->h_aux);
  {
    std::lock_guard<std::mutex> g(g_q_mu);
    g_q.plain -= ctx->plan.q_plain;
    g_q.high -= ctx->plan.q_high;
    g_q.masked -= ctx->plan.q_masked;
  }
  delete ctx;  // (its DevArrays free their memory here, on the device selected above)
  return LB_OK;
}

const char* lb_last_error(const lb_ctx* ctx) {
  // (a copy per calling thread: valid until that thread's next lb_last_error)
  static thread_local std::string out;
  out = ctx ? std::string(ctx->err) : g_create_err;
  return out.c_str();
}

int lb_scratch_per_queue(int device, uint64_t* out_bytes, uint32_t* out_lane_bytes) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0 || device < 0 || device >= n) return LB_ERR_NO_DEVICE;
  if (!out_bytes) return LB_ERR_INVALID_ARGUMENT;
  if (hipSetDevice(device) != hipSuccess) return LB_ERR_DEVICE;
  DeviceFacts dev;
  *out_bytes = scratch_per_queue(device, &dev);
  if (out_lane_bytes) *out_lane_bytes = dev.lane_bytes;
  return LB_OK;
}

int lb_slots(const lb_ctx* ctx) { return ctx ? ctx->plan.n_slots : 0; }
int lb_hw_queues(const lb_ctx* ctx) { return ctx ? ctx->plan.hw_queues : 0; }
int lb_last_call_streams(const lb_ctx* ctx) { return ctx ? ctx->last_call_streams : 0; }
int lb_last_latency_clocks(const lb_ctx* ctx, uint64_t* out4) {
  if (!ctx || !out4) return LB_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < 4; i++) out4[i] = ctx->lp_clk[i];
  return LB_OK;
}

#ifdef LB_COUNT_OPS
// Fp products executed per stage of the last completed verify call (count build only)
int lb_opcount_stages(const lb_ctx* ctx, unsigned long long* out, int max_stages) {
  if (!ctx) return 0;
  int n = 0;
  for (int i = 0; i < ctx->n_stages && n < max_stages; i++) out[n++] = ctx->stage_ops[i];
  return n;
}
#endif

int lb_last_stage_times(const lb_ctx* ctx, float* out_ms, const char** out_names, int max_stages) {
  if (!ctx) return 0;
  int n = ctx->n_stages < max_stages ? ctx->n_stages : max_stages;
  for (int i = 0; i < n; i++) {
    if (out_ms) out_ms[i] = ctx->stage_ms[i];
    if (out_names) out_names[i] = ctx->stage_name[i];
  }
  return ctx->n_stages;
}

// the priority lane used within the last prio_hold_ms (LB_PRIO_DYN)
static bool prio_active(lb_ctx* ctx) {
  const int64_t now = std::chrono::duration_cast<std::chrono::nanoseconds>(
                          std::chrono::steady_clock::now().time_since_epoch()).count();
  return ctx->plan.prio_dyn && (double)(now - ctx->last_prio_ns.load(std::memory_order_relaxed)) < ctx->plan.prio_hold_ms * 1e6;
}

// A call about to run on slot sl (idle: finish_slot has retired its last call): with
// LB_PRIO_DYN, the masked streams while the priority lane is in use, else the full ones.
// The priority slot marks the lane in use.
static void pick_streams(lb_ctx* ctx, Slot& sl) {
  if (&sl == &ctx->prio()) {
    ctx->last_prio_ns.store(std::chrono::duration_cast<std::chrono::nanoseconds>(
                                std::chrono::steady_clock::now().time_since_epoch()).count(),
                            std::memory_order_relaxed);
    return;
  }
  if (!ctx->plan.prio_dyn) return;
  if (prio_active(ctx)) {
    const Slot& m = ctx->slots[ctx->plan.mask_slot[&sl - ctx->slots]];
    sl.st[0] = m.st_mask[0];
    sl.st[1] = m.st_mask[1];
  } else {
    sl.st[0] = sl.st_full[0];
    sl.st[1] = sl.st_full[1];
  }
  // a synchronous call's borrowed second stream (BorrowGuard) stays: the call runs as
  // the two-stream DAG whichever stream pair slot 0 takes
  if (sl.guard_st) sl.st[1] = sl.guard_st;
}

// a two-phase call's record (LB_TP_RELEASE; the legacy mode keeps only the ticket ring)
static void tp_record(lb_ctx* ctx, uint64_t ticket, const lb_request_batch* b, const lb_key_source* ks, bool device,
                      uint8_t* valid, uint8_t* err, uint8_t* sst) {
  if (!ctx->cfg.tp_release) return;
  // (the ticket ring too: a finish of a ticket whose record was reused -- finished or waited
  // for by then, tp_reusable -- is a no-op, not an error)
  ctx->two_phase[ctx->two_phase_pos] = ticket;
  ctx->two_phase_pos = (ctx->two_phase_pos + 1) % lb_ctx::kTwoPhaseRing;
  TwoPhaseRec& r = ctx->tp[ticket % lb_ctx::kTwoPhaseRing];
  r.ticket = ticket;
  r.device = device;
  r.finished = r.have_partial = r.failed = r.waited = false;
  r.rerun = 0;
  r.batch = *b;
  r.by_keys = ks != nullptr;
  r.keys = ks ? *ks : lb_key_source{};
  r.valid = valid;
  r.err = err;
  r.sst = sst;
  if (!b->n_requests) {  // an empty shard: its partial is 1, known now
    memset(r.partial, 0, LB_GT_BYTES);
    r.partial[47] = 1;
    r.have_partial = true;
  }
}

static TwoPhaseRec* tp_find(lb_ctx* ctx, uint64_t ticket) {
  TwoPhaseRec& r = ctx->tp[ticket % lb_ctx::kTwoPhaseRing];
  // (records exist only for calls submitted in the release mode, whatever the mode now)
  return (ticket && r.ticket == ticket) ? &r : nullptr;
}

// A record may be overwritten once nothing about its call can change: it was waited for, or
// it was finished (with a submitted re-run, if any, retired).  Before that its outputs hold
// provisional verdicts that only its record turns into final ones.
static bool tp_reusable(lb_ctx* ctx, const TwoPhaseRec& r) {
  if (!r.ticket || r.waited) return true;
  return r.finished && !r.failed && (!r.rerun || !slot_of_ticket(ctx, r.rerun));
}

static int submit_device(lb_ctx* ctx, Slot& sl, const lb_request_batch* b, uint8_t* d_valid, uint8_t* d_req_err,
                         uint8_t* d_set_status, bool partial, uint64_t* out_ticket) {
  LB_TRY(finish_slot(ctx, sl));  // at most kSlots calls in flight
  pick_streams(ctx, sl);
  if (!partial) borrow_idle_stream(ctx, sl);  // (a pending two-phase call never holds a lent slot)
  LB_TRY(ensure_ws(ctx, sl, pipeline_ws_bytes(ctx, b->n_requests, b->n_sets)));
  Slab ws{sl.d_ws, 0, sl.ws_cap};
  LB_TRY(begin_call(ctx, sl));
  if (b->n_requests)
    LB_TRY(run_pipeline(ctx, sl, b->n_requests, b->n_sets, b->request_offsets, b->pubkeys, b->pk_offsets,
                        b->pubkey_indices, b->messages, b->signatures, b->sig_offsets, b->seed, d_valid, d_req_err,
                        d_set_status, ws, partial));
  else if (partial) {  // nothing to verify: the partial is the identity (1 in Fp12)
    memset(sl.h_partial, 0, LB_GT_BYTES);
    sl.h_partial[47] = 1;
    LB_HIP(hipEventRecord(sl.partial_ev, sl.st[0]));
    sl.ps = PipeState{};
    sl.partial_pending = !ctx->cfg.tp_release;
  }
  LB_TRY(end_call_async(ctx, sl));
  *out_ticket = sl.ticket;
  if (partial) tp_record(ctx, sl.ticket, b, nullptr, true, d_valid, d_req_err, d_set_status);
  return LB_OK;
}

// Host-side checks of a host-buffer batch: offsets must be monotone and start
// at 0 (a kernel must never index out of bounds).
static int check_host_batch(lb_ctx* ctx, const lb_request_batch* b) {
  const uint32_t nr = b->n_requests, ns = b->n_sets;
  if (b->request_offsets[0] != 0 || b->request_offsets[nr] != ns) {
    ctx->err = "request_offsets must start at 0 and end at n_sets";
    return LB_ERR_INVALID_ARGUMENT;
  }
  for (uint32_t k = 0; k < nr; k++)
    if (b->request_offsets[k + 1] < b->request_offsets[k]) {
      ctx->err = "request_offsets not monotone";
      return LB_ERR_INVALID_ARGUMENT;
    }
  if (b->sig_offsets[0] != 0) {
    ctx->err = "sig_offsets must start at 0";
    return LB_ERR_INVALID_ARGUMENT;
  }
  for (uint32_t i = 0; i < ns; i++)
    if (b->sig_offsets[i + 1] < b->sig_offsets[i]) {
      ctx->err = "sig_offsets not monotone";
      return LB_ERR_INVALID_ARGUMENT;
    }
  if (const uint32_t* pk_off = b->pk_offsets) {
    if (pk_off[0] != 0) {
      ctx->err = "pk_offsets must start at 0";
      return LB_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t i = 0; i < ns; i++)
      if (pk_off[i + 1] < pk_off[i]) {
        ctx->err = "pk_offsets not monotone";
        return LB_ERR_INVALID_ARGUMENT;
      }
  }
  return LB_OK;
}

// Host-buffer call on slot `sl`: inputs staged through the slot's pinned
// buffer (one H2D copy), the pipeline, verdicts copied back into pinned memory
// on the slot's stream and into the caller's buffers when the call retires.
// LB_HOST_TRACE=1: host-side phases of every host-buffer submission on stderr (ms)
static bool host_trace() {
  static const int on = [] {
    const char* e = getenv("LB_HOST_TRACE");
    return e && atoi(e) ? 1 : 0;
  }();
  return on != 0;
}
static double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// The keys each of n_sets descriptors names, counted into pk_off[0 .. n_sets] (running sums),
// with every bound the expansion's reads depend on checked: the kind, the list and a + len
// within it, the pool, the bits' bytes.  A BITS set counts the set bits below len.
static int count_set_keys(lb_ctx* ctx, uint32_t n_sets, const lb_set_keys* sets, uint32_t n_pool, const uint8_t* bits,
                          uint32_t n_bits_bytes, uint32_t* pk_off) {
  uint64_t total = 0;
  pk_off[0] = 0;
  for (uint32_t i = 0; i < n_sets; i++) {
    const lb_set_keys& d = sets[i];
    uint32_t cnt = 0;
    const char* why = nullptr;
    if (d.kind == LB_KEYS_DIRECT) {
      cnt = 1;
    } else if (d.kind == LB_KEYS_SLICE) {
      if ((uint64_t)d.a + d.len > n_pool) why = "a + len beyond key_pool";
      cnt = d.len;
    } else if (d.kind == LB_KEYS_BITS) {
      const uint32_t full = d.len / 8, tail = d.len & 7;
      if (d.list >= LB_INDEX_LISTS || ctx->lists[d.list].n == 0)
        why = "unknown or unloaded index list";
      else if ((uint64_t)d.a + d.len > ctx->lists[d.list].n)
        why = "a + len beyond the index list";
      else if ((uint64_t)d.bits_off + full + (tail ? 1 : 0) > n_bits_bytes)
        why = "bits_off + ceil(len / 8) beyond n_bits_bytes";
      else {
        const uint8_t* p = bits + d.bits_off;
        uint32_t k = 0;
        for (; k + 8 <= full; k += 8) {
          uint64_t w;
          memcpy(&w, p + k, 8);
          cnt += (uint32_t)__builtin_popcountll(w);
        }
        for (; k < full; k++) cnt += (uint32_t)__builtin_popcount(p[k]);
        if (tail) cnt += (uint32_t)__builtin_popcount(p[full] & ((1u << tail) - 1));
      }
    } else {
      why = "unknown kind";
    }
    if (!why && (total += cnt) > 0x7fffffffu) why = "more than 2^31 keys";
    if (why) {
      ctx->err = "lb_key_source: set " + std::to_string(i) + ": " + why;
      return LB_ERR_INVALID_ARGUMENT;
    }
    pk_off[i + 1] = (uint32_t)total;
  }
  return LB_OK;
}

static IndexLists index_lists(const lb_ctx* ctx) {
  IndexLists L;
  for (int i = 0; i < LB_INDEX_LISTS; i++) L.d[i] = ctx->lists[i].d;
  return L;
}

// ks (lb_verify_requests_keys*): the sets' keys by descriptor.  The key source is staged behind
// the package (layout_key_source), counted from the staged copy -- the counts size the indices
// and are the pk_offsets -- and expanded on the slot's stream in front of the pipeline, which
// then runs as for a call with pubkey_indices.
static int submit_host(lb_ctx* ctx, Slot& sl, const lb_request_batch* b, const lb_key_source* ks, uint8_t* out_valid,
                       uint8_t* out_req_err, uint8_t* out_set_status, bool partial, uint64_t* out_ticket) {
  const auto t0 = std::chrono::steady_clock::now();
  double t_check = 0, t_finish = 0, t_stage = 0, t_pipe = 0;
  const uint32_t nr = b->n_requests, ns = b->n_sets;
  LB_TRY(check_host_batch(ctx, b));
  t_check = ms_since(t0);
  const uint32_t* pk_off = b->pk_offsets;
  const size_t n_pk = ks ? 0 : pk_off ? pk_off[ns] : ns;
  const bool by_index = ks || b->pubkey_indices != nullptr;
  // mixed package: rows of `pubkeys` named by flagged indices (every row < n_rows is staged)
  size_t n_rows = 0;
  if (by_index && b->pubkeys)
    for (size_t k = 0; k < n_pk; k++) {
      const uint32_t j = b->pubkey_indices[k];
      if ((j & LB_PK_ROW_FLAG) && (size_t)(j & LB_PK_ROW_MASK) + 1 > n_rows) n_rows = (j & LB_PK_ROW_MASK) + 1;
    }
  // the package's arrays, declared once (layout_host_call): staged, copied and bound by HostBuf
  const HostCallShape shape{nr, ns, n_pk, b->sig_offsets[ns], n_rows, ks || pk_off != nullptr, by_index};
  const HostCallLayout lay = layout_host_call(shape);
  // (a keys call: HB_PKO is written below from the counts, HB_PK is empty)
  const void* const src[HB_INPUTS] = {b->request_offsets, pk_off,
                                      by_index ? (const void*)b->pubkey_indices : (const void*)b->pubkeys,
                                      b->messages, b->sig_offsets, b->signatures, b->seed, b->pubkeys};
  KeyShape kshape;
  KeyLayout klay{};
  if (ks) {
    kshape.n_sets = ns;
    kshape.n_pool = ks->n_pool;
    kshape.n_bits_bytes = ks->n_bits_bytes;
    klay = layout_key_source(kshape, lay.end);
  }
  LB_TRY(finish_slot(ctx, sl));
  pick_streams(ctx, sl);
  t_finish = ms_since(t0);
  if (!partial) borrow_idle_stream(ctx, sl);
  LB_TRY(ensure_pin(ctx, sl, ks ? klay.in_end : lay.end));
  char* h = sl.h_pin;
  for (int i = 0; i < HB_INPUTS; i++)
    if (lay.size[i] && src[i]) memcpy(h + lay.off[i], src[i], lay.size[i]);
  if (ks) {
    const void* const ksrc[KB_INPUTS] = {ks->sets, ks->key_pool, ks->bits};
    for (int i = 0; i < KB_INPUTS; i++)
      if (klay.size[i]) memcpy(h + klay.off[i], ksrc[i], klay.size[i]);
    uint32_t* h_pko = slab_at<uint32_t>(h, lay.off[HB_PKO]);
    const int rc = count_set_keys(ctx, ns, slab_at<const lb_set_keys>(h, klay.off[KB_SETS]), ks->n_pool,
                                  slab_at<const uint8_t>(h, klay.off[KB_BITS]), ks->n_bits_bytes, h_pko);
    if (rc != LB_OK) {  // refused with nothing enqueued
      release_borrowed(sl);
      return rc;
    }
    kshape.n_keys = h_pko[ns];
    klay = layout_key_source(kshape, lay.end);
  }
  const size_t io_end = ks ? klay.end : lay.end;
  LB_TRY(ensure_ws(ctx, sl, io_end + pipeline_ws_bytes(ctx, nr, ns)));
  Slab ws{sl.d_ws, io_end, sl.ws_cap};
  char* d = sl.d_ws;
  t_stage = ms_since(t0);
  LB_TRY(begin_call(ctx, sl));
  sl.dv_valid = slab_at<uint8_t>(d, lay.off[HB_VALID]);
  sl.dv_err = slab_at<uint8_t>(d, lay.off[HB_ERR]);
  sl.dv_sst = slab_at<uint8_t>(d, lay.off[HB_SST]);
  sl.hv_valid = slab_at<uint8_t>(h, lay.off[HB_VALID]);
  sl.hv_err = slab_at<uint8_t>(h, lay.off[HB_ERR]);
  sl.hv_sst = slab_at<uint8_t>(h, lay.off[HB_SST]);
  sl.out_valid = out_valid;
  sl.out_err = out_req_err;
  sl.out_sst = out_set_status;
  sl.out_nr = nr;
  sl.out_ns = out_set_status ? ns : 0;
  // (a keys call: one copy up to the end of the key source -- the few output bytes in between
  // travel with it and are written by the call before anything reads them)
  LB_TRY(slot_copy(ctx, sl, d, h, ks ? klay.in_end : lay.in_bytes, hipMemcpyHostToDevice, sl.st[0]));
  const auto in8 = [&](HostBuf i) { return slab_at<const uint8_t>(d, lay.off[i]); };
  const auto in32 = [&](HostBuf i) { return slab_at<const uint32_t>(d, lay.off[i]); };
  const uint32_t* d_pk_idx = by_index ? in32(HB_PK) : nullptr;
  if (ks) {
    uint32_t* d_idx = slab_at<uint32_t>(d, klay.off[KB_IDX]);
    if (ns)
      LB_STAGE("expand_keys", 0, k_expand_keys, blocks_for(ns, LB_LISTS_TPB / 64), LB_LISTS_TPB, ns,
               slab_at<const lb_set_keys>(d, klay.off[KB_SETS]), slab_at<const uint32_t>(d, klay.off[KB_POOL]),
               slab_at<const uint8_t>(d, klay.off[KB_BITS]), index_lists(ctx), in32(HB_PKO), d_idx);
    d_pk_idx = d_idx;
  }
  if (nr) {
    LB_TRY(run_pipeline(ctx, sl, nr, ns, in32(HB_REQ), by_index ? in8(HB_ROWS) : in8(HB_PK), in32(HB_PKO), d_pk_idx,
                        in8(HB_MSG), in8(HB_SIG), in32(HB_SIGO), in8(HB_SEED), sl.dv_valid, sl.dv_err, sl.dv_sst, ws,
                        partial));
    t_pipe = ms_since(t0);
  } else if (partial) {
    memset(sl.h_partial, 0, LB_GT_BYTES);
    sl.h_partial[47] = 1;
    LB_HIP(hipEventRecord(sl.partial_ev, sl.st[0]));
    sl.ps = PipeState{};
    sl.partial_pending = !ctx->cfg.tp_release;
  }
  LB_TRY(end_call_async(ctx, sl));
  *out_ticket = sl.ticket;
  if (partial) tp_record(ctx, sl.ticket, b, ks, false, out_valid, out_req_err, out_set_status);
  if (host_trace())
    fprintf(stderr, "lb_host_trace sets=%u check=%.3f finish_slot=%.3f stage=%.3f pipeline=%.3f total=%.3f dag=%d slot=%d\n",
            ns, t_check, t_finish, t_stage, t_pipe, ms_since(t0), sl.st[1] != sl.st[0] ? 1 : 0,
            (int)(&sl - ctx->slots));
  return LB_OK;
}

static void fill_stats(lb_ctx* ctx, uint64_t ticket, lb_verify_stats* stats) {
  if (!stats) return;
  const TicketStats& ts = ctx->tstats[ticket % lb_ctx::kTicketRing];
  if (ts.ticket == ticket) {
    stats->batch_retries = ts.batch_retries;
    stats->batch_sigs_success = ts.batch_sigs_success;
    stats->device_ms = ts.wall_ms;
  } else {  // more than kTicketRing calls retired since: the stats are gone
    *stats = lb_verify_stats{0, 0, 0.0};
  }
}

// Round robin over the slots, passing over a slot whose two-phase call still
// waits for the host's combined verdict (reusing it would retire that call with
// merged_ok = 0: correct verdicts, but every request's tail re-run); only when
// every slot holds a pending partial is the next one taken anyway.
static Slot& next_async_slot(lb_ctx* ctx) {  // internal: not part of the C ABI
  int s = ctx->next_slot;
  for (int k = 0; k < ctx->plan.n_slots; k++) {
    const int c = (ctx->next_slot + k) % ctx->plan.n_slots;
    if (!ctx->slots[c].partial_pending) {
      s = c;
      break;
    }
  }
  ctx->next_slot = (s + 1) % ctx->plan.n_slots;
  return ctx->slots[s];
}

int lb_verify_requests_device_async(lb_ctx* ctx, const lb_request_batch* b, uint8_t* d_valid, uint8_t* d_req_err,
                                    uint8_t* d_set_status, uint64_t* out_ticket) {
  if (!ctx || !out_ticket) return LB_ERR_INVALID_ARGUMENT;
  LB_TRY(validate_batch(ctx, b));
  if (!d_valid || !d_req_err) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(sm_pump(ctx));
  return submit_device(ctx, next_async_slot(ctx), b, d_valid, d_req_err, d_set_status, false, out_ticket);
}

// The host-buffer entry points, by pubkeys / indices (ks == nullptr) or by key source
static int host_async(lb_ctx* ctx, const lb_request_batch* b, const lb_key_source* ks, uint8_t* out_valid,
                      uint8_t* out_req_err, uint8_t* out_set_status, uint64_t* out_ticket) {
  if (!ctx || !out_ticket) return LB_ERR_INVALID_ARGUMENT;
  LB_TRY(validate_host_batch(ctx, b, ks));
  if (!out_valid || !out_req_err) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(sm_pump(ctx));
  return submit_host(ctx, next_async_slot(ctx), b, ks, out_valid, out_req_err, out_set_status, false, out_ticket);
}
int lb_verify_requests_async(lb_ctx* ctx, const lb_request_batch* b, uint8_t* out_valid, uint8_t* out_req_err,
                             uint8_t* out_set_status, uint64_t* out_ticket) {
  return host_async(ctx, b, nullptr, out_valid, out_req_err, out_set_status, out_ticket);
}
int lb_verify_requests_keys_async(lb_ctx* ctx, const lb_request_batch* b, const lb_key_source* ks, uint8_t* out_valid,
                                  uint8_t* out_req_err, uint8_t* out_set_status, uint64_t* out_ticket) {
  if (!ks) return LB_ERR_INVALID_ARGUMENT;
  return host_async(ctx, b, ks, out_valid, out_req_err, out_set_status, out_ticket);
}

static int host_partial(lb_ctx* ctx, const lb_request_batch* b, const lb_key_source* ks, uint32_t flags,
                        uint8_t* out_valid, uint8_t* out_req_err, uint8_t* out_set_status, uint64_t* out_ticket) {
  if (!ctx || !out_ticket) return LB_ERR_INVALID_ARGUMENT;
  LB_TRY(validate_host_batch(ctx, b, ks));
  if (!out_valid || !out_req_err) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(sm_pump(ctx));
  ctx->cfg.tp_release = ctx->cfg.tp_release_cfg && ctx->tp_pause == 0;
  if (ctx->tp_pause) ctx->tp_pause--;
  if (ctx->cfg.tp_release && !tp_reusable(ctx, ctx->tp[ctx->next_ticket % lb_ctx::kTwoPhaseRing])) {
    // (the ticket this call would take is end_call_async's next_ticket: no ticket is issued
    // in between)
    ctx->err = "two-phase ring full: the call " +
               std::to_string(ctx->tp[ctx->next_ticket % lb_ctx::kTwoPhaseRing].ticket) +
               " is neither finished nor waited for (" + std::to_string(lb_ctx::kTwoPhaseRing) +
               "-entry ring by ticket): finish or wait for older two-phase calls first";
    return LB_ERR_RESOURCES;
  }
  Slot& sl = next_async_slot(ctx);
  if (flags & LB_BATCH_DEVICE)
    return submit_device(ctx, sl, b, out_valid, out_req_err, out_set_status, true, out_ticket);
  return submit_host(ctx, sl, b, ks, out_valid, out_req_err, out_set_status, true, out_ticket);
}
int lb_verify_requests_partial_async(lb_ctx* ctx, const lb_request_batch* b, uint32_t flags, uint8_t* out_valid,
                                     uint8_t* out_req_err, uint8_t* out_set_status, uint64_t* out_ticket) {
  return host_partial(ctx, b, nullptr, flags, out_valid, out_req_err, out_set_status, out_ticket);
}
int lb_verify_requests_keys_partial_async(lb_ctx* ctx, const lb_request_batch* b, const lb_key_source* ks,
                                          uint8_t* out_valid, uint8_t* out_req_err, uint8_t* out_set_status,
                                          uint64_t* out_ticket) {
  if (!ks) return LB_ERR_INVALID_ARGUMENT;
  return host_partial(ctx, b, ks, 0, out_valid, out_req_err, out_set_status, out_ticket);
}

int lb_partial_wait(lb_ctx* ctx, uint64_t ticket, uint8_t* out576) {
  if (!ctx || !out576) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  Slot* sl = slot_of_ticket(ctx, ticket);
  if (TwoPhaseRec* r = tp_find(ctx, ticket)) {  // released: on its slot, or saved when it retired
    if (!r->have_partial && sl) {
      LB_HIP(hipEventSynchronize(sl->partial_ev));
      memcpy(out576, sl->h_partial, LB_GT_BYTES);
      return LB_OK;
    }
    if (r->have_partial) {
      memcpy(out576, r->partial, LB_GT_BYTES);
      return LB_OK;
    }
  }
  if (!sl || !sl->partial_pending) {
    ctx->err = "ticket is not a pending two-phase call";
    return LB_ERR_INVALID_ARGUMENT;
  }
  LB_HIP(hipEventSynchronize(sl->partial_ev));
  memcpy(out576, sl->h_partial, LB_GT_BYTES);
  return LB_OK;
}

int lb_partial_poll(lb_ctx* ctx, uint64_t ticket, int32_t* out_ready) {
  if (!ctx || !out_ready) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  Slot* sl = slot_of_ticket(ctx, ticket);
  if (TwoPhaseRec* r = tp_find(ctx, ticket)) {
    if (r->have_partial) {
      *out_ready = 1;
      return LB_OK;
    }
    if (sl) {
      const hipError_t q = hipEventQuery(sl->partial_ev);
      if (q == hipErrorNotReady) {
        *out_ready = 0;
        return LB_OK;
      }
      LB_HIP(q);
      *out_ready = 1;
      return LB_OK;
    }
  }
  if (!sl || !sl->partial_pending) {
    ctx->err = "ticket is not a pending two-phase call";
    return LB_ERR_INVALID_ARGUMENT;
  }
  const hipError_t q = hipEventQuery(sl->partial_ev);
  if (q == hipErrorNotReady) {
    *out_ready = 0;
    return LB_OK;
  }
  LB_HIP(q);
  *out_ready = 1;
  return LB_OK;
}

int lb_verify_requests_finish(lb_ctx* ctx, uint64_t ticket, int merged_ok) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  if (TwoPhaseRec* r = tp_find(ctx, ticket)) {
    if (r->finished) return LB_OK;
    r->finished = true;
    if (merged_ok) return LB_OK;  // its verdicts (every request not already false valid) stand
    // the combined check failed: the shard again as a one-phase call -- its own merged check
    // fails and every request is verified alone (worker.ts:74-85) -- into the same outputs,
    // after the released call has retired (its verdicts must not land after the re-run's)
    // (a failure from here on leaves the outputs provisional: the record says so, and
    // lb_wait returns the error instead of them)
    r->failed = true;
    ctx->tp_pause = ctx->ccfg.tp_pause;  // (the next two-phase calls: legacy mode)
    if (Slot* sl = slot_of_ticket(ctx, ticket)) LB_TRY(finish_slot(ctx, *sl));
    if (ctx->ccfg.fault_rerun) {  // (fault injection for the tests: the re-run's submission fails)
      ctx->err = "LB_FAULT_RERUN: the failed combine's re-verification was not submitted";
      return LB_ERR_DEVICE;
    }
    const lb_request_batch b = r->batch;
    uint8_t *v = r->valid, *e = r->err, *st = r->sst;
    const bool device = r->device;
    const lb_key_source keys = r->keys;
    const lb_key_source* ks = r->by_keys ? &keys : nullptr;
    uint64_t t2 = 0;
    LB_TRY(device ? submit_device(ctx, next_async_slot(ctx), &b, v, e, st, false, &t2)
                  : submit_host(ctx, next_async_slot(ctx), &b, ks, v, e, st, false, &t2));
    if (TwoPhaseRec* r2 = tp_find(ctx, ticket)) {
      r2->rerun = t2;
      r2->failed = false;
    }
    return LB_OK;
  }
  Slot* sl = slot_of_ticket(ctx, ticket);
  if (!sl || !sl->partial_pending) {
    // a two-phase call another call's slot reuse already resumed (with merged_ok
    // = 0: every request re-verified alone, so its verdicts stand): nothing to do
    for (int i = 0; ticket != 0 && i < lb_ctx::kTwoPhaseRing; i++)
      if (ctx->two_phase[i] == ticket) return LB_OK;
    // older than every two-phase ticket the ring still holds (the ring wrapped): whether
    // it was a two-phase call is no longer known, but any retired call's verdicts are
    // final, so finishing it is a no-op rather than an error
    const uint64_t oldest = ctx->two_phase[ctx->two_phase_pos];  // (0 until the ring wraps)
    if (ticket != 0 && oldest != 0 && ticket < oldest && ticket < ctx->next_ticket) return LB_OK;
    ctx->err = "ticket is not a two-phase call";
    return LB_ERR_INVALID_ARGUMENT;
  }
  if (!merged_ok && ctx->cfg.tp_release_cfg) ctx->tp_pause = ctx->ccfg.tp_pause;  // (failures go on: stay legacy)
  return finish_partial(ctx, *sl, merged_ok != 0);
}

int lb_gt_check(lb_ctx* ctx, uint32_t n, const uint8_t* partials576, int32_t* out_is_one) {
  if (!ctx || !out_is_one || (n && !partials576)) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  // (+ the combined product's 12 records for the round-program final exponentiation)
  const size_t need = (((size_t)n * LB_GT_BYTES + 255) & ~(size_t)255) + 256 + 12 * 64;
  if (ctx->ccfg.gt_lp) LB_TRY(lp_ensure(ctx));
  if (need > ctx->aux_cap) {
    LB_HIP(hipStreamSynchronize(ctx->aux_stream));
    if (ctx->d_aux) LB_HIP(hipFree(ctx->d_aux));
    if (ctx->h_aux) LB_HIP(hipHostFree(ctx->h_aux));
    ctx->d_aux = nullptr;
    ctx->h_aux = nullptr;
    ctx->aux_cap = 0;
    const size_t cap = need < 16 * LB_GT_BYTES + 256 + 12 * 64 ? 16 * LB_GT_BYTES + 256 + 12 * 64 : need;
    if (hipMalloc(&ctx->d_aux, cap) != hipSuccess || hipHostMalloc(&ctx->h_aux, cap, hipHostMallocDefault) != hipSuccess) {
      ctx->err = "gt_check buffers";
      return LB_ERR_OUT_OF_MEMORY;
    }
    ctx->aux_cap = cap;
  }
  uint8_t* d_out = ctx->d_aux;
  uint8_t* d_in = ctx->d_aux + 256;
  if (n) {
    memcpy(ctx->h_aux + 256, partials576, (size_t)n * LB_GT_BYTES);
    LB_HIP(hipMemcpyAsync(d_in, ctx->h_aux + 256, (size_t)n * LB_GT_BYTES, hipMemcpyHostToDevice, ctx->aux_stream));
  }
  if (ctx->ccfg.gt_lp) {
    // the product (one wave), then the final exponentiation as a round program on one
    // workgroup (~420 rounds) instead of the one-wave chain
    uint32_t* d_rec = reinterpret_cast<uint32_t*>(ctx->d_aux + 256 + (((size_t)n * LB_GT_BYTES + 255) & ~(size_t)255));
    LB_ENQUEUE(ctx->aux_stream, k_gt_prod, 1, TPB, n, (const uint8_t*)d_in, d_rec, d_out);
    LB_ENQUEUE(ctx->aux_stream, k_lp_final_lane, 1, LB_LP_TPB,
               (const uint32_t*)(ctx->d_lp.d + LB_LP_PROGS[LB_LP_PROG_FINAL_LANE].off), (const uint32_t*)d_rec, d_out);
  } else {
    LB_ENQUEUE(ctx->aux_stream, k_gt_check, 1, TPB, n, (const uint8_t*)d_in, d_out);
  }
  LB_HIP(hipMemcpyAsync(ctx->h_aux, d_out, 2, hipMemcpyDeviceToHost, ctx->aux_stream));
  LB_HIP(hipStreamSynchronize(ctx->aux_stream));
  if (ctx->h_aux[1]) {
    ctx->err = "partial with a coefficient >= p";
    return LB_ERR_INVALID_ARGUMENT;
  }
  *out_is_one = ctx->h_aux[0] ? 1 : 0;
  return LB_OK;
}

int lb_poll(lb_ctx* ctx, uint64_t ticket, int32_t* out_done) {
  if (!ctx || !out_done) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(sm_pump(ctx));
  *out_done = 1;
  if (TwoPhaseRec* r = tp_find(ctx, ticket)) {
    if (!r->finished) {  // (lb_wait would first finish it with merged_ok = 0)
      *out_done = 0;
      return LB_OK;
    }
    if (r->rerun) ticket = r->rerun;
  }
  Slot* sl = slot_of_ticket(ctx, ticket);
  if (!sl) return LB_OK;  // retired
  // (a same-message package's phase 1 still running: sm_pump above found it unfinished;
  // in phase 2 its retries' end event decides)
  if (sl->partial_pending || (sl->sm.active && sl->sm.phase == 1)) {
    *out_done = 0;
    return LB_OK;
  }
  const hipError_t q = hipEventQuery(sl->done);
  if (q == hipErrorNotReady) {
    *out_done = 0;
    return LB_OK;
  }
  LB_HIP(q);
  return LB_OK;
}

int lb_wait(lb_ctx* ctx, uint64_t ticket, lb_verify_stats* stats) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(sm_pump(ctx));
  bool rerun = false;
  if (TwoPhaseRec* r = tp_find(ctx, ticket)) {
    // waited for without a combined verdict: as before, each request verified alone
    if (!r->finished) {
      const int rc = lb_verify_requests_finish(ctx, ticket, 0);
      if (rc != LB_OK) {
        if (TwoPhaseRec* r2 = tp_find(ctx, ticket)) r2->waited = true;
        return rc;
      }
    }
    TwoPhaseRec* r2 = tp_find(ctx, ticket);
    if (r2 && r2->failed) {  // the failed combine's re-run never ran: the outputs are not verdicts
      const uint64_t own = ticket;
      if (Slot* sl = slot_of_ticket(ctx, own)) LB_TRY(finish_slot(ctx, *sl));
      r2->waited = true;
      ctx->err = "two-phase call " + std::to_string(own) +
                 ": the combined check failed and its re-verification could not be submitted; its outputs are not "
                 "verdicts";
      return LB_ERR_DEVICE;
    }
    if (r2) r2->waited = true;
    if (r2 && r2->rerun) {
      ticket = r2->rerun;
      rerun = true;
    }
  }
  if (Slot* sl = slot_of_ticket(ctx, ticket)) LB_TRY(finish_slot(ctx, *sl));
  fill_stats(ctx, ticket, stats);
  // a re-run after a failed combined check: the shard's batch failed once and every request
  // was verified alone (worker.ts:74-85 counts that as one retry of the merged batch)
  if (rerun && stats) {
    stats->batch_retries = 1;
    stats->batch_sigs_success = 0;
  }
  return LB_OK;
}

int lb_verify_requests_device(lb_ctx* ctx, const lb_request_batch* b, uint8_t* d_valid, uint8_t* d_req_err,
                              uint8_t* d_set_status, lb_verify_stats* stats) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  LB_TRY(validate_batch(ctx, b));
  if (!d_valid || !d_req_err) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  uint64_t t = 0;
  if (b->n_sets <= ctx->cfg.lp_max_sets && !(lp_lone_rule(ctx->cfg, b->n_sets) && !any_slot_busy(ctx))) {
    // latency path: the priority lane, beside any calls in flight
    LB_TRY(submit_device(ctx, ctx->prio(), b, d_valid, d_req_err, d_set_status, false, &t));
    return lb_wait(ctx, t, stats);
  }
  BorrowGuard g{ctx};
  LB_TRY(borrow_second_stream(ctx, g));
  LB_TRY(submit_device(ctx, ctx->slots[0], b, d_valid, d_req_err, d_set_status, false, &t));  // slot 0: DAG
  return lb_wait(ctx, t, stats);
}

static int host_sync(lb_ctx* ctx, const lb_request_batch* b, const lb_key_source* ks, uint8_t* out_valid,
                     uint8_t* out_req_err, uint8_t* out_set_status, lb_verify_stats* stats) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  LB_TRY(validate_host_batch(ctx, b, ks));
  if (!out_valid || !out_req_err) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  if (b->n_requests == 0) {
    if (stats) *stats = lb_verify_stats{0, 0, 0.0};
    return LB_OK;
  }
  uint64_t t = 0;
  if (b->n_sets <= ctx->cfg.lp_max_sets && !(lp_lone_rule(ctx->cfg, b->n_sets) && !any_slot_busy(ctx))) {
    // latency path: the priority lane, beside any calls in flight
    LB_TRY(submit_host(ctx, ctx->prio(), b, ks, out_valid, out_req_err, out_set_status, false, &t));
    return lb_wait(ctx, t, stats);
  }
  BorrowGuard g{ctx};  // synchronous host API: slot 0 (two-stream DAG, lowest latency)
  LB_TRY(borrow_second_stream(ctx, g));
  LB_TRY(submit_host(ctx, ctx->slots[0], b, ks, out_valid, out_req_err, out_set_status, false, &t));
  return lb_wait(ctx, t, stats);
}
int lb_verify_requests(lb_ctx* ctx, const lb_request_batch* b, uint8_t* out_valid, uint8_t* out_req_err,
                       uint8_t* out_set_status, lb_verify_stats* stats) {
  return host_sync(ctx, b, nullptr, out_valid, out_req_err, out_set_status, stats);
}
int lb_verify_requests_keys(lb_ctx* ctx, const lb_request_batch* b, const lb_key_source* ks, uint8_t* out_valid,
                            uint8_t* out_req_err, uint8_t* out_set_status, lb_verify_stats* stats) {
  if (!ks) return LB_ERR_INVALID_ARGUMENT;
  return host_sync(ctx, b, ks, out_valid, out_req_err, out_set_status, stats);
}

static int host_priority(lb_ctx* ctx, const lb_request_batch* b, const lb_key_source* ks, uint8_t* out_valid,
                         uint8_t* out_req_err, uint8_t* out_set_status, uint64_t* out_ticket) {
  if (!ctx || !out_ticket) return LB_ERR_INVALID_ARGUMENT;
  LB_TRY(validate_host_batch(ctx, b, ks));
  if (!out_valid || !out_req_err) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(sm_pump(ctx));
  return submit_host(ctx, ctx->prio(), b, ks, out_valid, out_req_err, out_set_status, false, out_ticket);
}
int lb_verify_requests_priority_async(lb_ctx* ctx, const lb_request_batch* b, uint8_t* out_valid,
                                      uint8_t* out_req_err, uint8_t* out_set_status, uint64_t* out_ticket) {
  return host_priority(ctx, b, nullptr, out_valid, out_req_err, out_set_status, out_ticket);
}
int lb_verify_requests_keys_priority_async(lb_ctx* ctx, const lb_request_batch* b, const lb_key_source* ks,
                                           uint8_t* out_valid, uint8_t* out_req_err, uint8_t* out_set_status,
                                           uint64_t* out_ticket) {
  if (!ks) return LB_ERR_INVALID_ARGUMENT;
  return host_priority(ctx, b, ks, out_valid, out_req_err, out_set_status, out_ticket);
}
// ---- helpers for small host-buffer calls ----------------------------------
// A synchronous helper call on the idle slot 0: the call declares its buffers (bls_carve.h),
// begin() selects the device, retires the calls in flight, sizes and carves slot 0's slab from
// the list and uploads the inputs on ctx->stream; the call launches; end() downloads the
// outputs and synchronises once.  A call that wants its time in lb_last_stage_times names its
// stages as it launches: stage() closes the stage before it and opens the next on ctx->stream,
// stage_end() closes the last (end() does, ahead of the downloads, when the call has not), and
// end() publishes them.  The first stage() clears the stages published before, whether or not
// ccfg.stage_events has any event recorded; a call that names no stage leaves them alone.
// Stages follow one another without a gap.  A call may launch again after end() and call it a
// second time for what those launches wrote (kzg_finish_verify).
// (The longest list is kzg_prove's: 16 buffers.)
struct HelperCall : Carve<24> {
  lb_ctx* ctx;
  const char* stage_name[lb_ctx::kHelperStages] = {};
  int n_staged = 0;
  bool stage_open = false;
  explicit HelperCall(lb_ctx* c) : ctx(c) {}
  int stage(const char* name) {
    if (n_staged == lb_ctx::kHelperStages) {
      ctx->err = "more stages than the helper calls' clock has events for";
      return LB_ERR_INVALID_ARGUMENT;
    }
    if (n_staged == 0) ctx->n_stages = 0;
    if (ctx->ccfg.stage_events) LB_HIP(hipEventRecord(ctx->helper_ev[n_staged], ctx->stream));
    stage_name[n_staged++] = name;
    stage_open = true;
    return LB_OK;
  }
  int stage_end() {
    if (stage_open && ctx->ccfg.stage_events) LB_HIP(hipEventRecord(ctx->helper_ev[n_staged], ctx->stream));
    stage_open = false;
    return LB_OK;
  }
  int begin() {
    LB_HIP(hipSetDevice(ctx->device));
    LB_TRY(helper_slot(ctx));
    LB_TRY(ensure_ws(ctx, layout()));
    Slot& sl = ctx->slots[0];
    if (!fits(sl.ws_cap)) {
      ctx->err = "workspace overflow";
      return LB_ERR_OUT_OF_MEMORY;
    }
    bind(sl.d_ws);
    for (int i = 0; i < n; i++)
      if (buf[i].kind == CARVE_IN && buf[i].bytes && buf[i].src)
        LB_HIP(hipMemcpyAsync(sl.d_ws + buf[i].off, buf[i].src, buf[i].bytes, hipMemcpyHostToDevice, ctx->stream));
    return LB_OK;
  }
  int end() {
    LB_TRY(stage_end());
    const Slot& sl = ctx->slots[0];
    for (int i = 0; i < n; i++)
      if (buf[i].kind == CARVE_OUT && buf[i].bytes && buf[i].dst)
        LB_HIP(hipMemcpyAsync(buf[i].dst, sl.d_ws + buf[i].off, buf[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
    LB_HIP(hipStreamSynchronize(ctx->stream));
    if (!ctx->ccfg.stage_events) return LB_OK;
    for (int i = 0; i < n_staged; i++) {
      LB_HIP(hipEventElapsedTime(&ctx->stage_ms[i], ctx->helper_ev[i], ctx->helper_ev[i + 1]));
      ctx->stage_name[i] = stage_name[i];
      ctx->stage_ops[i] = 0;
    }
    if (n_staged) ctx->n_stages = n_staged;
    return LB_OK;
  }
};

int lb_hash_to_g2(lb_ctx* ctx, uint32_t n, const uint8_t* messages, uint8_t* out192) {
  if (!ctx || (n && (!messages || !out192))) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  HelperCall c(ctx);
  auto d_msg = c.in(messages, (size_t)n * 32);
  auto d_h = c.scratch<g2a>(n);
  auto d_out = c.out(out192, (size_t)n * 192);
  LB_TRY(c.begin());
  LB_LAUNCH(k_hash, blocks_for(n), TPB, n, d_msg, d_h);
  LB_LAUNCH(k_g2a_serialize, blocks_for(n), TPB, n, (const g2a*)d_h, d_out);
  return c.end();
}

int lb_decode_signatures(lb_ctx* ctx, uint32_t n, const uint8_t* sigs, const uint32_t* sig_off, uint8_t* out_status,
                         uint8_t* out192) {
  if (!ctx || (n && (!sigs || !sig_off || !out_status))) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  for (uint32_t i = 0; i < n; i++)
    if (sig_off[i + 1] < sig_off[i]) return LB_ERR_INVALID_ARGUMENT;
  HelperCall c(ctx);
  auto d_s = c.in(sigs, sig_off[n]);
  auto d_o = c.in(sig_off, (size_t)n + 1);
  auto d_sig = c.scratch<g2j>(n);
  auto d_st = c.out(out_status, n);
  auto d_out = c.out(out192, (size_t)n * 192);  // (out192 is optional: serialized all the same)
  LB_TRY(c.begin());
  LB_LAUNCH(k_decode_sigs, blocks_for(n), TPB, n, d_s, d_o, (const uint8_t*)nullptr, d_sig, d_st);
  LB_LAUNCH(k_g2_serialize, blocks_for(n), TPB, n, (const g2j*)d_sig, d_out);
  return c.end();
}

// One aggregated key from `src` (n keys by bytes or by table index): Jacobian sum, serialized
// (dev_indices: the indices where they already lie in HBM, a stretch of an index list)
static int aggregate_pubkeys(lb_ctx* ctx, uint32_t n, const uint8_t* pks, const uint32_t* indices, uint8_t* out96,
                             uint8_t* out_status, const uint32_t* dev_indices = nullptr) {
  HelperCall c(ctx);
  const uint32_t off[2] = {0, n};
  uint8_t st = 0;
  auto d_p = c.in(pks, (size_t)n * 96, pks != nullptr);
  auto d_idx = c.in(indices, n, indices != nullptr);
  auto d_off = c.in(off, 2);
  auto d_pk = c.scratch<g1j>(1);
  auto d_out = c.out(out96, 96);
  auto d_st = c.out(&st, 1);
  LB_TRY(c.begin());
  const bool by_index = indices || dev_indices;
  const PkSource src{d_p, dev_indices ? dev_indices : (const uint32_t*)d_idx, by_index ? ctx->table.d : nullptr,
                     by_index ? ctx->table.n : 0};
  LB_LAUNCH(k_pubkeys_single, 1, TPB, 1u, src, d_off, d_pk, d_st);
  LB_LAUNCH(k_pubkeys_agg, 1, TPB, 1u, src, d_off, d_pk, d_st);
  LB_LAUNCH(k_g1_serialize, 1, TPB, 1u, (const g1j*)d_pk, d_out);
  LB_TRY(c.end());
  if (st == LB_ST_PK_INFINITY) st = LB_ST_OK;  // an infinite aggregate is a valid encoding (0x40...)
  if (out_status) *out_status = st;
  return LB_OK;
}

int lb_aggregate_pubkeys(lb_ctx* ctx, uint32_t n, const uint8_t* pks, uint8_t* out96, uint8_t* out_status) {
  if (!ctx || !out96 || (n && !pks)) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) {
    ctx->err = "EMPTY_AGGREGATE_ARRAY";
    return LB_ERR_INVALID_ARGUMENT;
  }
  return aggregate_pubkeys(ctx, n, pks, nullptr, out96, out_status);
}

int lb_pubkeys_from_bytes(lb_ctx* ctx, uint32_t n, const uint8_t* pks, uint32_t pk_len, uint8_t* out96,
                          uint8_t* out_status) {
  if (!ctx || (n && (!pks || !out96 || !out_status)) || (pk_len != 48 && pk_len != 96)) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  HelperCall c(ctx);
  auto d_in = c.in(pks, (size_t)n * pk_len);
  auto d_out = c.out(out96, (size_t)n * 96);
  auto d_st = c.out(out_status, n);
  LB_TRY(c.begin());
  LB_LAUNCH(k_pubkey_validate, blocks_for(n), TPB, n, d_in, pk_len, d_out, d_st);
  return c.end();
}

// ---- device-resident pubkey table (index2pubkey mirror) ------------------------
int lb_pubkey_table_append(lb_ctx* ctx, uint32_t n, const uint8_t* pks, uint32_t pk_len, int32_t* out_bad_index) {
  if (!ctx || (n && !pks) || (pk_len != 48 && pk_len != 96)) return LB_ERR_INVALID_ARGUMENT;
  if (out_bad_index) *out_bad_index = -1;
  if (n == 0) return LB_OK;
  if ((uint64_t)ctx->table.n + n > 0x7fffffffu) {
    ctx->err = "pubkey table full";
    return LB_ERR_INVALID_ARGUMENT;
  }
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(helper_slot(ctx));  // calls in flight read the table
  const uint32_t need = ctx->table.n + n;
  LB_TRY(ctx->table.reserve(ctx, need, ctx->table.n));
  // decode straight into the table tail, in chunks that bound the staging workspace;
  // table_n only advances once every key decoded
  const uint32_t chunk = 1u << 20;
  std::vector<uint8_t> st;
  for (uint32_t first = 0; first < n; first += chunk) {
    const uint32_t m = n - first < chunk ? n - first : chunk;
    st.resize(m);
    HelperCall c(ctx);
    auto d_in = c.in(pks + (size_t)first * pk_len, (size_t)m * pk_len);
    auto d_st = c.out(st.data(), m);
    LB_TRY(c.begin());
    LB_LAUNCH(k_table_decode, blocks_for(m), TPB, m, d_in, pk_len, ctx->table.d + ctx->table.n + first, d_st);
    LB_TRY(c.end());
    for (uint32_t i = 0; i < m; i++)
      if (st[i] != LB_ST_OK) {
        if (out_bad_index) *out_bad_index = (int32_t)(first + i);
        ctx->err = "pubkey fails PublicKey.fromBytes (bad encoding / not on curve)";
        return LB_ERR_INVALID_ARGUMENT;
      }
  }
  ctx->table.n = need;
  return LB_OK;
}

int lb_pubkey_table_size(const lb_ctx* ctx, uint32_t* out_n) {
  if (!ctx || !out_n) return LB_ERR_INVALID_ARGUMENT;
  *out_n = ctx->table.n;
  return LB_OK;
}

int lb_pubkey_table_truncate(lb_ctx* ctx, uint32_t n) {
  if (!ctx || n > ctx->table.n) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(helper_slot(ctx));
  ctx->table.n = n;
  return LB_OK;
}

int lb_pubkey_table_read(lb_ctx* ctx, uint32_t first, uint32_t n, uint8_t* out96) {
  if (!ctx || (n && !out96) || (uint64_t)first + n > ctx->table.n) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  HelperCall c(ctx);
  auto d_out = c.out(out96, (size_t)n * 96);
  LB_TRY(c.begin());
  LB_LAUNCH(k_g1a_serialize, blocks_for(n), TPB, n, (const g1a*)(ctx->table.d + first), d_out);
  return c.end();
}

int lb_aggregate_pubkeys_indexed(lb_ctx* ctx, uint32_t n, const uint32_t* indices, uint8_t* out96,
                                 uint8_t* out_status) {
  if (!ctx || !out96 || (n && !indices)) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) {
    ctx->err = "EMPTY_AGGREGATE_ARRAY";
    return LB_ERR_INVALID_ARGUMENT;
  }
  return aggregate_pubkeys(ctx, n, nullptr, indices, out96, out_status);
}

// ---- device-resident index lists (shufflings, sync committees) -------------------
// (a list that is written takes all new contents: reserve keeps none of the old)
int lb_index_list_put(lb_ctx* ctx, uint32_t list, uint32_t n, const uint32_t* indices) {
  if (!ctx || list >= LB_INDEX_LISTS || (n && !indices)) return LB_ERR_INVALID_ARGUMENT;
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(helper_slot(ctx));  // calls in flight read the lists
  lb_ctx::IndexList& L = ctx->lists[list];
  if (n) {
    LB_TRY(L.reserve(ctx, n, 0));
    LB_TRY(L.upload(ctx, 0, indices, n));
    LB_HIP(hipStreamSynchronize(ctx->stream));
  }
  L.n = n;
  return LB_OK;
}

int lb_index_list_shuffle(lb_ctx* ctx, uint32_t list, uint32_t n, const uint32_t* active, const uint8_t* seed32,
                          uint32_t* out_shuffling) {
  if (!ctx || list >= LB_INDEX_LISTS || (n && !active) || !seed32) return LB_ERR_INVALID_ARGUMENT;
  if (n > LB_SHUFFLE_MAX) {
    ctx->err = "lb_index_list_shuffle: more than LB_SHUFFLE_MAX indices";
    return LB_ERR_INVALID_ARGUMENT;
  }
  if (n <= 1) {  // nothing to swap: a plain upload, no stage
    ctx->n_stages = 0;
    LB_TRY(lb_index_list_put(ctx, list, n, active));
    if (n && out_shuffling) out_shuffling[0] = active[0];
    return LB_OK;
  }
  const uint32_t n_digests = LB_SHUFFLE_ROUNDS * ((n + 255) / 256);
  HelperCall c(ctx);
  auto d_active = c.in(active, n);
  auto d_seed = c.in(seed32, 32);
  auto d_pivots = c.scratch<uint32_t>(LB_SHUFFLE_ROUNDS);
  auto d_table = c.scratch<uint32_t>((size_t)n_digests * 8);  // [round][ceil(n/256)] digests
  LB_TRY(c.begin());
  lb_ctx::IndexList& L = ctx->lists[list];
  LB_TRY(L.reserve(ctx, n, 0));  // (begin() has retired the calls in flight, which may read the list)
  LB_TRY(c.stage("shuffle"));
  LB_LAUNCH(k_shuffle_sources, blocks_for(n_digests, LB_LISTS_TPB), LB_LISTS_TPB, n, d_seed, d_pivots, d_table);
  LB_LAUNCH(k_shuffle_apply, blocks_for(n, LB_LISTS_TPB), LB_LISTS_TPB, n, (const uint32_t*)d_pivots,
            (const uint8_t*)(uint32_t*)d_table, d_active, L.d);
  LB_TRY(c.stage_end());
  L.n = 0;  // (until the kernels are known to have run)
  if (out_shuffling) LB_TRY(L.download(ctx, 0, out_shuffling, n));
  LB_TRY(c.end());
  L.n = n;
  return LB_OK;
}

int lb_index_list_size(const lb_ctx* ctx, uint32_t list, uint32_t* out_n) {
  if (!ctx || list >= LB_INDEX_LISTS || !out_n) return LB_ERR_INVALID_ARGUMENT;
  *out_n = ctx->lists[list].n;
  return LB_OK;
}

int lb_index_list_read(lb_ctx* ctx, uint32_t list, uint32_t first, uint32_t n, uint32_t* out) {
  if (!ctx || list >= LB_INDEX_LISTS || (n && !out) || (uint64_t)first + n > ctx->lists[list].n)
    return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(ctx->lists[list].download(ctx, first, out, n));
  LB_HIP(hipStreamSynchronize(ctx->stream));
  return LB_OK;
}

int lb_aggregate_pubkeys_list(lb_ctx* ctx, uint32_t list, uint32_t first, uint32_t n, uint8_t* out96,
                              uint8_t* out_status) {
  if (!ctx || !out96 || list >= LB_INDEX_LISTS) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) {
    ctx->err = "EMPTY_AGGREGATE_ARRAY";
    return LB_ERR_INVALID_ARGUMENT;
  }
  if ((uint64_t)first + n > ctx->lists[list].n) {
    ctx->err = "lb_aggregate_pubkeys_list: first + n beyond the index list";
    return LB_ERR_INVALID_ARGUMENT;
  }
  return aggregate_pubkeys(ctx, n, nullptr, nullptr, out96, out_status, ctx->lists[list].d + first);
}

// ---- device-resident balance table (EffectiveBalanceIncrements mirror) -----------------
int lb_balance_table_put(lb_ctx* ctx, uint32_t first, uint32_t n, const uint8_t* increments) {
  if (!ctx || (n && !increments)) return LB_ERR_INVALID_ARGUMENT;
  if (first > ctx->bal.n || (uint64_t)first + n > 0x7fffffffu) {
    ctx->err = "lb_balance_table_put: first beyond the table's size";
    return LB_ERR_INVALID_ARGUMENT;
  }
  if (n == 0) return LB_OK;
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(helper_slot(ctx));  // (nothing in flight reads the table; the order of calls is kept all the same)
  const uint32_t need = first + n;
  LB_TRY(ctx->bal.reserve(ctx, need, ctx->bal.n));
  LB_TRY(ctx->bal.upload(ctx, first, increments, n));
  LB_HIP(hipStreamSynchronize(ctx->stream));
  if (need > ctx->bal.n) ctx->bal.n = need;
  return LB_OK;
}

int lb_balance_table_size(const lb_ctx* ctx, uint32_t* out_n) {
  if (!ctx || !out_n) return LB_ERR_INVALID_ARGUMENT;
  *out_n = ctx->bal.n;
  return LB_OK;
}

int lb_balance_table_read(lb_ctx* ctx, uint32_t first, uint32_t n, uint8_t* out) {
  if (!ctx || (n && !out) || (uint64_t)first + n > ctx->bal.n) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(ctx->bal.download(ctx, first, out, n));
  LB_HIP(hipStreamSynchronize(ctx->stream));
  return LB_OK;
}

// ---- balance-weighted sampling: proposers, the sync committee (k_sample.hip) -------------
// The size of the pass behind one of `pass` candidates per seed: twice it, within
// LB_SAMPLE_PASS_MAX and 2^20 candidates over all seeds (the scratch of a pass: 5 bytes each)
static uint32_t sample_next_pass(uint32_t pass, uint32_t n_seeds) {
  uint32_t cap = (1u << 20) / n_seeds;  // (n_seeds <= 64: at least 16,384, a multiple of 64)
  if (cap > LB_SAMPLE_PASS_MAX) cap = LB_SAMPLE_PASS_MAX;
  return pass * 2 < cap ? pass * 2 : cap;
}

int lb_sample_by_balance(lb_ctx* ctx, uint32_t n_seeds, const uint8_t* seeds32, uint32_t count, uint32_t n,
                         const uint32_t* active, uint32_t max_inc, uint32_t max_candidates, uint32_t store_list,
                         uint32_t* out_indices, uint32_t* out_found, uint32_t* out_tried) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  if (n_seeds == 0) return LB_OK;
  const char* why = nullptr;
  if (!seeds32 || !active || !out_indices)
    why = "a null buffer";
  else if (n == 0)
    why = "no active indices";
  else if (count == 0)
    why = "count == 0";
  else if (n_seeds > LB_SAMPLE_MAX_SEEDS)
    why = "more than LB_SAMPLE_MAX_SEEDS seeds";
  else if (count > LB_SAMPLE_MAX_COUNT)
    why = "count above LB_SAMPLE_MAX_COUNT";
  else if (n > LB_SHUFFLE_MAX)
    why = "more than LB_SHUFFLE_MAX indices";
  else if (max_inc < 1 || max_inc > 255)
    why = "max_increment outside [1, 255]";
  else if (max_candidates < 1 || max_candidates > LB_SAMPLE_MAX_CANDIDATES)
    why = "max_candidates outside [1, LB_SAMPLE_MAX_CANDIDATES]";
  else if (store_list != LB_NO_LIST && store_list >= LB_INDEX_LISTS)
    why = "unknown index list";
  else if (store_list != LB_NO_LIST && n_seeds != 1)
    why = "a list is stored from one seed";
  if (why) {
    ctx->err = std::string("lb_sample_by_balance: ") + why;
    return LB_ERR_INVALID_ARGUMENT;
  }
  // the largest pass this call can come to, which is its last: the scratch is carved once
  // (the first pass is at most 4,096 and the bound at least 16,384, so no pass is smaller than the one before)
  uint32_t pass = LB_SAMPLE_FIRST_PASS(count), pass_max = pass;
  for (uint32_t seen = pass; seen < max_candidates; seen += pass_max) pass_max = sample_next_pass(pass_max, n_seeds);
  HelperCall c(ctx);
  auto d_active = c.in(active, n);
  auto d_seeds = c.in(seeds32, (size_t)n_seeds * 32);
  auto d_pivots = c.scratch<uint32_t>((size_t)n_seeds * LB_SHUFFLE_ROUNDS);
  auto d_state = c.scratch<uint32_t>(1 + 2 * (size_t)n_seeds);  // max index; found[]; tried[]
  auto d_out = c.out(out_indices, (size_t)n_seeds * count);
  auto d_cand = c.scratch<uint32_t>((size_t)n_seeds * pass_max);
  auto d_acc = c.scratch<uint8_t>((size_t)n_seeds * pass_max);
  LB_TRY(c.begin());
  uint32_t* const d_max = d_state;
  uint32_t* const d_found = d_max + 1;
  uint32_t* const d_tried = d_found + n_seeds;
  LB_TRY(c.stage("sample"));
  LB_HIP(hipMemsetAsync(d_state, 0, sizeof(uint32_t) * (1 + 2 * (size_t)n_seeds), ctx->stream));
  LB_HIP(hipMemsetAsync(d_out, 0xff, sizeof(uint32_t) * (size_t)n_seeds * count, ctx->stream));  // LB_SAMPLE_NONE
  const uint32_t range_blocks = blocks_for(n, LB_LISTS_TPB);
  LB_LAUNCH(k_sample_range, range_blocks < 1024u ? range_blocks : 1024u, LB_LISTS_TPB, n, d_active, d_max);
  LB_LAUNCH(k_sample_pivots, blocks_for(n_seeds * LB_SHUFFLE_ROUNDS, LB_LISTS_TPB), LB_LISTS_TPB, n_seeds, n, d_seeds,
            d_pivots);
  uint32_t state[1 + 2 * LB_SAMPLE_MAX_SEEDS];
  uint32_t* const found = state + 1;
  for (uint32_t base = 0; base < max_candidates; base += pass, pass = sample_next_pass(pass, n_seeds)) {
    LB_ENQUEUE(ctx->stream, k_sample_candidates, dim3(blocks_for(pass, LB_LISTS_TPB), n_seeds), LB_LISTS_TPB, n, count,
               base, pass, max_candidates, max_inc, d_seeds, (const uint32_t*)d_pivots, d_active,
               (const uint8_t*)ctx->bal.d, ctx->bal.n, (const uint32_t*)d_found, d_cand, d_acc);
    LB_LAUNCH(k_sample_select, n_seeds, LB_LISTS_TPB, count, base, pass, (const uint32_t*)d_cand,
              (const uint8_t*)d_acc, d_out, d_found, d_tried);
    LB_HIP(hipMemcpyAsync(state, d_state, sizeof(uint32_t) * (1 + (size_t)n_seeds), hipMemcpyDeviceToHost,
                          ctx->stream));
    LB_HIP(hipStreamSynchronize(ctx->stream));
    if (state[0] >= ctx->bal.n) {  // (the candidates kernel read no increment outside the table)
      ctx->err = "lb_sample_by_balance: an active index at or beyond the balance table's size";
      return LB_ERR_INVALID_ARGUMENT;
    }
    bool filled = true;
    for (uint32_t s = 0; s < n_seeds; s++) filled = filled && found[s] >= count;
    if (filled) break;
  }
  LB_TRY(c.stage_end());
  if (store_list != LB_NO_LIST && found[0] == count) {  // device to device; an unfilled seed leaves the list
    lb_ctx::IndexList& L = ctx->lists[store_list];
    LB_TRY(L.reserve(ctx, count, 0));
    L.n = 0;  // (until the copy is known to have run)
    LB_HIP(hipMemcpyAsync(L.d, d_out, sizeof(uint32_t) * (size_t)count, hipMemcpyDeviceToDevice, ctx->stream));
    LB_HIP(hipStreamSynchronize(ctx->stream));
    L.n = count;
  }
  LB_HIP(hipMemcpyAsync(state + 1 + n_seeds, d_tried, sizeof(uint32_t) * (size_t)n_seeds, hipMemcpyDeviceToHost,
                        ctx->stream));
  LB_TRY(c.end());
  for (uint32_t s = 0; s < n_seeds; s++) {
    if (out_found) out_found[s] = found[s];
    if (out_tried) out_tried[s] = found[s] == count ? state[1 + n_seeds + s] : max_candidates;
  }
  return LB_OK;
}

int lb_expand_set_keys(lb_ctx* ctx, uint32_t n_sets, const lb_key_source* ks, uint32_t* out_pk_offsets,
                       uint32_t* out_indices, uint32_t max_indices) {
  if (!ctx || !ks || !out_pk_offsets || (n_sets && !ks->sets) || (ks->n_pool && !ks->key_pool) ||
      (ks->n_bits_bytes && !ks->bits) || (max_indices && !out_indices))
    return LB_ERR_INVALID_ARGUMENT;
  std::vector<uint32_t> pk_off((size_t)n_sets + 1);
  LB_TRY(count_set_keys(ctx, n_sets, ks->sets, ks->n_pool, ks->bits, ks->n_bits_bytes, pk_off.data()));
  const uint32_t n_keys = pk_off[n_sets];
  if (n_keys > max_indices) {
    ctx->err = "lb_expand_set_keys: the sets expand to more than max_indices";
    return LB_ERR_INVALID_ARGUMENT;
  }
  memcpy(out_pk_offsets, pk_off.data(), sizeof(uint32_t) * pk_off.size());
  if (n_sets == 0) return LB_OK;
  HelperCall c(ctx);
  auto d_sets = c.in(ks->sets, n_sets);
  auto d_pool = c.in(ks->key_pool, ks->n_pool);
  auto d_bits = c.in(ks->bits, ks->n_bits_bytes);
  auto d_off = c.in(pk_off.data(), pk_off.size());
  auto d_idx = c.out(out_indices, n_keys);
  LB_TRY(c.begin());
  LB_LAUNCH(k_expand_keys, blocks_for(n_sets, LB_LISTS_TPB / 64), LB_LISTS_TPB, n_sets, d_sets, d_pool, d_bits,
            index_lists(ctx), d_off, d_idx);
  return c.end();
}

// ---- signing roots -----------------------------------------------------------
static int signing_roots(lb_ctx* ctx, uint32_t n, uint32_t m, const uint8_t* in, size_t in_per_obj,
                         const uint8_t* domains, uint32_t dstride, uint8_t* out32) {
  if (!ctx || (n && (!in || !domains || !out32)) || (dstride != 0 && dstride != 32)) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  HelperCall c(ctx);
  auto d_in = c.in(in, (size_t)n * in_per_obj);
  auto d_dom = c.in(domains, (dstride ? (size_t)n : 1) * 32);
  auto d_out = c.out(out32, (size_t)n * 32);
  LB_TRY(c.begin());
  if (m == 0)
    LB_LAUNCH(k_signing_root_att, blocks_for(n), TPB, n, d_in, d_dom, dstride, d_out);
  else
    LB_LAUNCH(k_signing_root_chunks, blocks_for(n), TPB, n, m, d_in, d_dom, dstride, d_out);
  return c.end();
}

int lb_signing_roots_attestation(lb_ctx* ctx, uint32_t n, const uint8_t* data128, const uint8_t* domains,
                                 uint32_t domain_stride, uint8_t* out32) {
  return signing_roots(ctx, n, 0, data128, 128, domains, domain_stride, out32);
}

int lb_signing_roots_attestation_device(lb_ctx* ctx, uint32_t n, const uint8_t* d_data, const uint8_t* d_domains,
                                        uint32_t dstride, uint8_t* d_out) {
  if (!ctx || (n && (!d_data || !d_domains || !d_out)) || (dstride != 0 && dstride != 32))
    return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(helper_slot(ctx));
  LB_LAUNCH(k_signing_root_att, blocks_for(n), TPB, n, d_data, d_domains, dstride, d_out);
  LB_HIP(hipStreamSynchronize(ctx->stream));
  return LB_OK;
}

int lb_signing_roots_chunks(lb_ctx* ctx, uint32_t n, uint32_t m, const uint8_t* chunks, const uint8_t* domains,
                            uint32_t domain_stride, uint8_t* out32) {
  if (m < 1 || m > 16) return LB_ERR_INVALID_ARGUMENT;
  return signing_roots(ctx, n, m, chunks, (size_t)m * 32, domains, domain_stride, out32);
}

int lb_aggregate_signatures(lb_ctx* ctx, uint32_t n, const uint8_t* sigs, const uint32_t* sig_off, uint8_t* out192,
                            int32_t* out_bad_index) {
  if (!ctx || !out192 || !out_bad_index || (n && (!sigs || !sig_off))) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) {
    ctx->err = "EMPTY_AGGREGATE_ARRAY";
    return LB_ERR_INVALID_ARGUMENT;
  }
  for (uint32_t i = 0; i < n; i++)
    if (sig_off[i + 1] < sig_off[i]) return LB_ERR_INVALID_ARGUMENT;
  std::vector<uint8_t> st(n);
  HelperCall c(ctx);
  auto d_s = c.in(sigs, sig_off[n]);
  auto d_o = c.in(sig_off, (size_t)n + 1);
  auto d_sig = c.scratch<g2j>(n);
  auto d_st = c.out(st.data(), n);
  auto d_sum = c.scratch<g2j>(1);
  auto d_out = c.out(out192, 192);
  LB_TRY(c.begin());
  LB_LAUNCH(k_decode_sigs, blocks_for(n), TPB, n, d_s, d_o, (const uint8_t*)nullptr, d_sig, d_st);
  LB_LAUNCH(k_jac_sum<fp2>, 1, 256, n, (const g2j*)d_sig, d_sum);
  LB_LAUNCH(k_g2_serialize, 1, TPB, 1u, (const g2j*)d_sum, d_out);
  LB_TRY(c.end());
  *out_bad_index = -1;
  for (uint32_t i = 0; i < n; i++)
    if (st[i] != LB_ST_OK) {
      *out_bad_index = (int32_t)i;
      break;
    }
  return LB_OK;
}

// Same-message jobs, batched (BlsMultiThreadWorkerPool.verifySignatureSetsSameMessage
// jobs: jobItemWorkReq sameMessage, jobItem.ts:64-86, the worker's verify of
// the aggregated set, index.ts:455-489, and the per-set retry of failed jobs,
// index.ts:473-484,557-568 / jobItemSameMessageToMultiSet, jobItem.ts:93-125).
// Phase 1 (sm_submit): every signature decoded + validated ONCE, pubkeys and
// signatures summed per job, every job's aggregated set verified as a 1-set
// request of ONE merged call.  Phase 2 (sm_complete, when the call retires and
// only if a job failed): the sets of the failed jobs, each its own 1-set
// request, through the same pipeline on the same slot -- signatures from the
// phase-1 decode (k_sm_retry_gather), pubkeys / messages from the phase-1
// uploads: nothing re-packed or re-uploaded but the retry index list.
}  // extern "C"

// phase-2 inputs: retry r = set rset[r] of job rjob[r] as a 1-set request
__global__ void __launch_bounds__(TPB) k_sm_retry_gather(uint32_t n, const uint32_t* __restrict__ rset,
                                                         const uint32_t* __restrict__ rjob,
                                                         const g2j* __restrict__ sig, const uint8_t* __restrict__ sst,
                                                         const uint8_t* __restrict__ msgs,
                                                         const uint32_t* __restrict__ pk_index, g2j* __restrict__ out_sig,
                                                         uint8_t* __restrict__ out_st, uint8_t* __restrict__ out_msg,
                                                         uint32_t* __restrict__ out_idx, uint32_t* __restrict__ out_req) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  const uint32_t i = rset[r], j = rjob[r];
  const g2j g = sig[i];
  uint8_t st = sst[i];
  // a 1-set request: core verify rejects the infinite signature (k_decode_sigs' single-set rule)
  if (st == LB_ST_OK && jac_is_inf(g)) st = LB_ST_ZERO_SIGNATURE;
  out_sig[r] = g;
  out_st[r] = st;
  for (int k = 0; k < 32; k++) out_msg[(size_t)r * 32 + k] = msgs[(size_t)j * 32 + k];
  // the set's key: its validator index, or row i of the package's 96-byte keys
  out_idx[r] = pk_index ? pk_index[i] : (i | LB_PK_ROW_FLAG);
  out_req[r] = r;
  if (r == n - 1) out_req[n] = n;
}

namespace {

int sm_validate(lb_ctx* ctx, const lb_same_message_batch* b) {
  const uint32_t nj = b->n_jobs, ns = b->n_sets;
  if (!b->job_offsets || !b->sig_offsets || !b->messages || !b->seed || (ns && !b->signatures) ||
      (ns && !b->pubkeys && !b->pubkey_indices)) {
    ctx->err = "null pointer in lb_same_message_batch";
    return LB_ERR_INVALID_ARGUMENT;
  }
  if (ctx->sm_mode == LB_SM_RANDOMIZED && ns >= LB_SM_AGG_INDEX_FLAG) {
    ctx->err = "randomized same-message aggregation: n_sets must be below 2^31 (LB_SM_AGG_INDEX_FLAG)";
    return LB_ERR_INVALID_ARGUMENT;
  }
  if (b->job_offsets[0] != 0 || b->job_offsets[nj] != ns || b->sig_offsets[0] != 0) {
    ctx->err = "job_offsets / sig_offsets must start at 0 (job_offsets end at n_sets)";
    return LB_ERR_INVALID_ARGUMENT;
  }
  for (uint32_t j = 0; j < nj; j++)
    if (b->job_offsets[j + 1] < b->job_offsets[j]) {
      ctx->err = "job_offsets not monotone";
      return LB_ERR_INVALID_ARGUMENT;
    }
  for (uint32_t i = 0; i < ns; i++)
    if (b->sig_offsets[i + 1] < b->sig_offsets[i]) {
      ctx->err = "sig_offsets not monotone";
      return LB_ERR_INVALID_ARGUMENT;
    }
  return LB_OK;
}

// A buffer of the same-message package on slot `sl`: offset `off` (SmLayout, bls_carve.h) of
// the slot's slab / of its pinned staging; nullptr for a buffer the package does not have
template <class T>
T* sm_d(const Slot& sl, size_t off) { return slab_at<T>(sl.d_ws, off); }
template <class T>
T* sm_h(const Slot& sl, size_t off) { return slab_at<T>(sl.h_pin, off); }

// The package's shape and its layout, and the slot's staging and slab sized for all of it --
// both phases, every set retried -- before anything is enqueued: nothing later can fail for
// space.  front_only: lb_same_message_aggregates (no verification, no phase 2).
int sm_prepare(lb_ctx* ctx, Slot& sl, const lb_same_message_batch* b, bool agg, bool front_only, SmShape& s,
               SmLayout& L) {
  const uint32_t nj = b->n_jobs, ns = b->n_sets;
  const bool by_index = b->pubkey_indices != nullptr;
  // mixed package (indices AND rows): rows of `pubkeys` named by flagged indices, as in
  // lb_request_batch (every row < n_rows is staged)
  size_t n_rows = 0;
  if (by_index && b->pubkeys)
    for (uint32_t i = 0; i < ns; i++) {
      const uint32_t j = b->pubkey_indices[i];
      if ((j & LB_PK_ROW_FLAG) && (size_t)(j & LB_PK_ROW_MASK) + 1 > n_rows) n_rows = (j & LB_PK_ROW_MASK) + 1;
    }
  s = SmShape{nj, ns, b->sig_offsets[ns], n_rows, by_index, agg, ns && ns <= LB_SM_DEC_MAX && ctx->ccfg.sm_lp_decode, front_only,
              front_only ? 0 : pipeline_ws_bytes(ctx, nj, nj), front_only ? 0 : pipeline_ws_bytes(ctx, ns, ns)};
  L = layout_same_message(s, ns);
  LB_TRY(ensure_pin(ctx, sl, L.pin_end));
  LB_TRY(ensure_ws(ctx, sl, L.ws_end));
  if (L.ws_end > sl.ws_cap || L.pin_end > sl.pin_cap) {
    ctx->err = "workspace overflow";
    return LB_ERR_OUT_OF_MEMORY;
  }
  return LB_OK;
}

// The front of phase 1 on slot `sl` (already retired by the caller, sized by sm_prepare), in
// aggregation mode `mode`: the package staged and uploaded, every signature decoded + validated
// once, each job's aggregated set in d_pk96 / d_sig192 with its flags d_jbad / d_jpkst.
int sm_front(lb_ctx* ctx, Slot& sl, const lb_same_message_batch* b, uint32_t mode, const SmShape& s,
             const SmLayout& L) {
  const uint32_t nj = b->n_jobs, ns = b->n_sets;
  const bool by_index = s.by_index;
  const bool randomized = mode == LB_SM_RANDOMIZED;
  const void* const src[SI_COUNT] = {b->job_offsets, by_index ? (const void*)b->pubkey_indices : (const void*)b->pubkeys,
                                     b->sig_offsets, b->signatures, b->messages, b->seed, nullptr, nullptr, b->pubkeys};
  for (int i = 0; i < SI_COUNT; i++)
    if (L.in_size[i] && src[i]) memcpy(sl.h_pin + L.in[i], src[i], L.in_size[i]);
  uint32_t *areq = sm_h<uint32_t>(sl, L.in[SI_AREQ]), *asig = sm_h<uint32_t>(sl, L.in[SI_ASIG]);
  for (uint32_t j = 0; j <= nj; j++) {
    areq[j] = j;        // every job one request of one (aggregated) set
    asig[j] = 192 * j;  // Signature.aggregate(...).toBytes(uncompressed)
  }
  const uint32_t* d_joff = sm_d<const uint32_t>(sl, L.in[SI_JOFF]);
  const uint8_t* d_pks = sm_d<const uint8_t>(sl, L.in[SI_PK]);
  const uint32_t* d_sigo = sm_d<const uint32_t>(sl, L.in[SI_SIGO]);
  const uint8_t* d_sigs = sm_d<const uint8_t>(sl, L.in[SI_SIG]);
  const uint8_t* d_seed = sm_d<const uint8_t>(sl, L.in[SI_SEED]);
  const uint8_t* d_rows = sm_d<const uint8_t>(sl, L.in[SI_ROWS]);
  g2j* d_sig = sm_d<g2j>(sl, L.d_sig);
  uint8_t* d_sst = sm_d<uint8_t>(sl, L.d_sst);
  g1j* d_jpk = sm_d<g1j>(sl, L.d_jpk);
  uint8_t* d_jpkst = sm_d<uint8_t>(sl, L.d_jpkst);
  uint8_t* d_pk96 = sm_d<uint8_t>(sl, L.d_pk96);
  uint8_t* d_sig192 = sm_d<uint8_t>(sl, L.d_sig192);
  uint8_t* d_jbad = sm_d<uint8_t>(sl, L.d_jbad);
  LB_TRY(begin_call(ctx, sl));
  LB_HIP(hipMemcpyAsync(sl.d_ws, sl.h_pin, L.in_bytes, hipMemcpyHostToDevice, sl.st[0]));
  const PkSource src_pk{by_index ? d_rows : d_pks, by_index ? (const uint32_t*)d_pks : nullptr, ctx->table.d,
                        ctx->table.n};
  const uint32_t agg_grid = nj < 16384u ? nj : 16384u;
  // randomized sums: the G1 side needs only the upload, so with a second stream it runs there,
  // beside the decode and the G2 side (joined below, before the aggregated sets are read)
  const int pk_st = randomized && sl.st[1] != sl.st[0] ? 1 : 0;
  if (randomized) {
    if (pk_st) LB_TRY(stream_wait(ctx, sl, 0, 1, 5));
    LB_STAGE("sm_rand_pk", pk_st, k_sm_rand_pk, agg_grid, TPB, nj, d_joff, src_pk, d_seed, d_jpk, d_jpkst, d_pk96);
  }
  if (s.dec) {
    // a small package: each signature's decode as a round program on an 8-row workgroup (~540
    // rounds) instead of k_decode_sigs' one-lane chain (~4 ms); the same outputs and statuses
    LB_TRY(lp_ensure(ctx));
    uint32_t* d_dec_in = sm_d<uint32_t>(sl, L.dec_in);
    uint32_t* d_dec_fl = sm_d<uint32_t>(sl, L.dec_fl);
    uint32_t* d_dec_out = sm_d<uint32_t>(sl, L.dec_out);
    uint32_t* d_dec_ofl = sm_d<uint32_t>(sl, L.dec_ofl);
    uint8_t* d_dec_pre = sm_d<uint8_t>(sl, L.dec_pre);
    LB_STAGE("sm_decode", 0, k_sm_dec_prep, blocks_for(ns, 256), 256u, ns, d_sigs, d_sigo, d_dec_in, d_dec_fl,
             d_dec_pre);
    LB_STAGE("sm_decode", 0, k_lp_dec, ns, LB_LP_DEC_ROWS * 16u, ctx->d_lp.d + LB_LP_PROGS[LB_LP_PROG_SIG_DECODE].off, ns,
             (const uint32_t*)d_dec_in, (const uint32_t*)d_dec_fl, d_dec_out, d_dec_ofl);
    LB_STAGE("sm_decode", 0, k_sm_dec_finish, blocks_for(ns, 256), 256u, ns, (const uint8_t*)d_dec_pre,
             (const uint32_t*)d_dec_in, (const uint32_t*)d_dec_fl, (const uint32_t*)d_dec_out,
             (const uint32_t*)d_dec_ofl, d_sig, d_sst, (const uint8_t*)nullptr);
  } else if (ns) {
    LB_STAGE("sm_decode", 0, k_decode_sigs, blocks_for(ns), TPB, ns, d_sigs, d_sigo, (const uint8_t*)nullptr, d_sig,
             d_sst);
  }
  if (randomized) {
    LB_STAGE("sm_rand_sig", 0, k_sm_rand_sig, agg_grid, TPB, nj, d_joff, d_seed, (const g2j*)d_sig,
             (const uint8_t*)d_sst, d_sig192, d_jbad);
    if (pk_st) LB_TRY(stream_wait(ctx, sl, 1, 0, 6));
  } else {
    LB_STAGE("sm_pubkeys", 0, k_pubkeys_single, blocks_for(nj), TPB, nj, src_pk, d_joff, d_jpk, d_jpkst);
    LB_STAGE("sm_pubkeys_agg", 0, k_pubkeys_agg, agg_grid, TPB, nj, src_pk, d_joff, d_jpk, d_jpkst);
    LB_STAGE("sm_aggregate", 0, k_same_message_agg, agg_grid, TPB, nj, d_joff, (const g2j*)d_sig,
             (const uint8_t*)d_sst, (const g1j*)d_jpk, d_pk96, d_sig192, d_jbad);
  }
  return LB_OK;
}

// The caller's side of an _agg call: the optional mask, the two outputs.
struct SmAggOut {
  const uint8_t* mask;
  uint8_t* sig96;
  uint32_t* count;
};

// A run of jobs per wave with about one wave of sets in it (k_job_sig: a job of 64 sets or more
// alone, up to LB_JS_JOBS small ones together).
inline uint32_t job_sig_jobs_per_wg(uint32_t n_jobs, uint64_t n_sets) {
  const uint64_t g = n_sets ? (uint64_t)TPB * n_jobs / n_sets : LB_JS_JOBS;
  return (uint32_t)(g < 1 ? 1 : g > LB_JS_JOBS ? LB_JS_JOBS : g);
}

// The stage sm_job_sig: every job's included signatures summed and compressed (k_aggsig.hip),
// copied into the call's pinned results.
int sm_job_sig(lb_ctx* ctx, Slot& sl, SmState& m) {
  const SmLayout& L = m.lay;
  const uint32_t jpw = job_sig_jobs_per_wg(m.nj, m.ns);
  const uint32_t runs = (m.nj + jpw - 1) / jpw;
  uint8_t* d_agg96 = sm_d<uint8_t>(sl, L.d_agg96);
  uint32_t* d_aggcnt = sm_d<uint32_t>(sl, L.d_aggcnt);
  LB_STAGE("sm_job_sig", 0, k_job_sig, runs < 16384u ? runs : 16384u, TPB, m.nj, jpw,
           sm_d<const uint32_t>(sl, L.in[SI_JOFF]), sm_d<const g2j>(sl, L.d_sig), sm_d<const uint8_t>(sl, L.d_inc),
           d_agg96, d_aggcnt);
  LB_HIP(hipMemcpyAsync(sm_h<uint8_t>(sl, L.h_agg96), d_agg96, (size_t)m.nj * 96, hipMemcpyDeviceToHost, sl.st[0]));
  LB_HIP(hipMemcpyAsync(sm_h<uint8_t>(sl, L.h_aggcnt), d_aggcnt, (size_t)m.nj * 4, hipMemcpyDeviceToHost, sl.st[0]));
  return LB_OK;
}

// Phase 1 on slot `sl` (already retired by the caller); the call stays busy
// until finish_slot, which runs sm_complete.
int sm_submit(lb_ctx* ctx, Slot& sl, const lb_same_message_batch* b, uint8_t* out_valid, uint8_t* out_job_fast,
              const SmAggOut* agg = nullptr) {
  const uint32_t nj = b->n_jobs, ns = b->n_sets;
  const uint32_t mode = ctx->sm_mode;  // read once: the call keeps it whatever the context does later
  SmState& m = sl.sm;
  LB_TRY(sm_prepare(ctx, sl, b, agg != nullptr, false, m.shape, m.lay));
  const SmLayout& L = m.lay;
  LB_TRY(sm_front(ctx, sl, b, mode, m.shape, L));
  uint8_t *d_valid = sm_d<uint8_t>(sl, L.d_valid), *d_err = sm_d<uint8_t>(sl, L.d_err);
  uint8_t *d_jbad = sm_d<uint8_t>(sl, L.d_jbad), *d_jpkst = sm_d<uint8_t>(sl, L.d_jpkst);
  m.agg = agg != nullptr;
  m.nj = nj;
  m.ns = ns;
  if (agg) {
    m.out_job_sig96 = agg->sig96;
    m.out_job_count = agg->count;
    m.masked = agg->mask != nullptr;
    if (agg->mask && ns) {
      memcpy(sm_h<uint8_t>(sl, L.h_mask), agg->mask, ns);
      LB_HIP(hipMemcpyAsync(sm_d<uint8_t>(sl, L.d_mask), sm_h<uint8_t>(sl, L.h_mask), ns, hipMemcpyHostToDevice,
                            sl.st[0]));
    }
  }
  Slab ws{sl.d_ws, L.pipe1, sl.ws_cap};
  LB_TRY(run_pipeline(ctx, sl, nj, nj, sm_d<const uint32_t>(sl, L.in[SI_AREQ]), sm_d<const uint8_t>(sl, L.d_pk96),
                      nullptr, nullptr, sm_d<const uint8_t>(sl, L.in[SI_MSG]), sm_d<const uint8_t>(sl, L.d_sig192),
                      sm_d<const uint32_t>(sl, L.in[SI_ASIG]), sm_d<const uint8_t>(sl, L.in[SI_SEED]), d_valid, d_err,
                      nullptr, ws));
  if (agg) {
    // behind phase 1: the include decision on the device (the host's fast-path rule), then the
    // jobs' sums -- final when no job is retried, else redone behind phase 2 (sm_advance_launch)
    if (ns)
      LB_STAGE("sm_job_sig", 0, k_sm_include, blocks_for(ns, 256), 256u, ns, nj, sm_d<const uint32_t>(sl, L.in[SI_JOFF]),
               (const uint8_t*)d_valid, (const uint8_t*)d_err, (const uint8_t*)d_jbad, (const uint8_t*)d_jpkst,
               m.masked ? sm_d<const uint8_t>(sl, L.d_mask) : nullptr, sm_d<uint8_t>(sl, L.d_inc));
    LB_TRY(sm_job_sig(ctx, sl, m));
  }
  LB_HIP(hipMemcpyAsync(sm_h<uint8_t>(sl, L.h_valid), d_valid, nj, hipMemcpyDeviceToHost, sl.st[0]));
  LB_HIP(hipMemcpyAsync(sm_h<uint8_t>(sl, L.h_err), d_err, nj, hipMemcpyDeviceToHost, sl.st[0]));
  LB_HIP(hipMemcpyAsync(sm_h<uint8_t>(sl, L.h_jbad), d_jbad, nj, hipMemcpyDeviceToHost, sl.st[0]));
  LB_HIP(hipMemcpyAsync(sm_h<uint8_t>(sl, L.h_jpkst), d_jpkst, nj, hipMemcpyDeviceToHost, sl.st[0]));
  m.active = true;
  m.phase = 1;
  m.mode = mode;
  m.out_valid = out_valid;
  m.out_job_fast = out_job_fast;
  return end_call_async(ctx, sl);
}

// Progress of a same-message call.  Phase 1 done: verdicts of the jobs whose
// aggregate passed, and phase 2 -- the sets of the other jobs, each its own
// 1-set request -- enqueued on the same slot at once (sm_pump launches it from
// any later library call, so it need not wait for the caller's lb_wait).
// Phase 2 done: its verdicts.  block = false: return at once when the phase's
// work is still in flight.
int sm_advance_launch(lb_ctx* ctx, Slot& sl, bool block);

// One step of a same-message call; a failure ends the call (sm.active cleared) and
// stays on its slot for its own ticket's wait to report.
int sm_advance(lb_ctx* ctx, Slot& sl, bool block) {
  const int rc = sm_advance_launch(ctx, sl, block);
  if (rc != LB_OK) {
    sl.sm.active = false;
    sl.sm.phase = 0;
    sl.sm.err = rc;
    sl.sm.err_msg = ctx->err;
  }
  return rc;
}

int sm_advance_launch(lb_ctx* ctx, Slot& sl, bool block) {
  SmState& m = sl.sm;
  if (!m.active) return LB_OK;
  if (!block) {
    const hipError_t q = hipEventQuery(sl.done);
    if (q == hipErrorNotReady) return LB_OK;
    if (q != hipSuccess) LB_HIP(q);
  }
  LB_HIP(hipEventSynchronize(sl.done));
  const uint32_t nj = m.nj, ns = m.ns;
  const SmLayout& L = m.lay;
  uint32_t* h_rset = sm_h<uint32_t>(sl, L.h_rset);  // set indices, then (from ns) job indices
  if (m.phase == 2) {
    const uint8_t *rv = sm_h<const uint8_t>(sl, L.h_rvalid), *re = sm_h<const uint8_t>(sl, L.h_rerr);
    for (uint32_t r = 0; r < m.nr; r++) m.out_valid[h_rset[r]] = (rv[r] && re[r] == LB_REQ_OK) ? 1 : 0;
  } else {
    const uint8_t *v = sm_h<const uint8_t>(sl, L.h_valid), *e = sm_h<const uint8_t>(sl, L.h_err),
                  *jb = sm_h<const uint8_t>(sl, L.h_jbad), *pst = sm_h<const uint8_t>(sl, L.h_jpkst);
    const uint32_t* h_joff = sm_h<const uint32_t>(sl, L.in[SI_JOFF]);
    uint32_t fast_sets = 0, retried_jobs = 0, nr = 0;
    for (uint32_t j = 0; j < nj; j++) {
      // fast path: aggregated set valid, every signature validated, pubkeys aggregated
      const bool fast = v[j] && e[j] == LB_REQ_OK && !jb[j] && pst[j] == LB_ST_OK;
      if (m.out_job_fast) m.out_job_fast[j] = fast ? 1 : 0;
      const uint32_t a = h_joff[j], b = h_joff[j + 1];
      if (fast) {
        for (uint32_t i = a; i < b; i++) m.out_valid[i] = 1;
        fast_sets += b - a;
      } else if (b > a) {
        retried_jobs++;
        for (uint32_t i = a; i < b; i++) {
          h_rset[nr] = i;
          h_rset[(size_t)ns + nr] = j;
          nr++;
        }
      }
    }
    m.nr = nr;
    m.retried_jobs = retried_jobs;
    m.fast_sets = fast_sets;
    if (nr) {
      // phase 2's buffers for nr retries: inside the slab sized at submit (layout_same_message)
      const SmLayout R = layout_same_message(m.shape, nr);
      const bool by_index = m.shape.by_index;
      uint32_t* d_rset = sm_d<uint32_t>(sl, R.d_rset);
      g2j* d_rsig = sm_d<g2j>(sl, R.d_rsig);
      uint8_t* d_rst = sm_d<uint8_t>(sl, R.d_rst);
      uint8_t* d_rmsg = sm_d<uint8_t>(sl, R.d_rmsg);
      uint32_t* d_ridx = sm_d<uint32_t>(sl, R.d_ridx);
      uint32_t* d_rreq = sm_d<uint32_t>(sl, R.d_rreq);
      uint8_t* d_rvalid = sm_d<uint8_t>(sl, R.d_rvalid);
      uint8_t* d_rerr = sm_d<uint8_t>(sl, R.d_rerr);
      const uint8_t* d_pks = sm_d<const uint8_t>(sl, L.in[SI_PK]);
      const uint8_t* d_mask = m.masked ? sm_d<const uint8_t>(sl, L.d_mask) : nullptr;
      Slab ws{sl.d_ws, R.pipe2, sl.ws_cap};
      LB_HIP(hipMemcpyAsync(d_rset, h_rset, sizeof(uint32_t) * 2 * (size_t)ns, hipMemcpyHostToDevice, sl.st[0]));
      LB_ENQUEUE(sl.st[0], k_sm_retry_gather, blocks_for(nr), TPB, nr, (const uint32_t*)d_rset,
                 (const uint32_t*)(d_rset + ns), sm_d<const g2j>(sl, L.d_sig), sm_d<const uint8_t>(sl, L.d_sst),
                 sm_d<const uint8_t>(sl, L.in[SI_MSG]), by_index ? (const uint32_t*)d_pks : (const uint32_t*)nullptr,
                 d_rsig, d_rst, d_rmsg, d_ridx, d_rreq);
      LB_TRY(run_pipeline(ctx, sl, nr, nr, d_rreq, by_index ? sm_d<const uint8_t>(sl, L.in[SI_ROWS]) : d_pks, nullptr,
                          d_ridx, d_rmsg, nullptr, nullptr, sm_d<const uint8_t>(sl, L.in[SI_SEED]), d_rvalid, d_rerr,
                          nullptr, ws, false, d_rsig, d_rst));
      LB_HIP(hipMemcpyAsync(sm_h<uint8_t>(sl, L.h_rvalid), d_rvalid, nr, hipMemcpyDeviceToHost, sl.st[0]));
      LB_HIP(hipMemcpyAsync(sm_h<uint8_t>(sl, L.h_rerr), d_rerr, nr, hipMemcpyDeviceToHost, sl.st[0]));
      if (m.agg) {  // behind phase 2: the retried sets that verified alone join the sums
        LB_STAGE("sm_job_sig", 0, k_sm_include_retry, blocks_for(nr, 256), 256u, nr, (const uint32_t*)d_rset,
                 (const uint8_t*)d_rvalid, (const uint8_t*)d_rerr, d_mask, sm_d<uint8_t>(sl, L.d_inc));
        LB_TRY(sm_job_sig(ctx, sl, m));
      }
      LB_TRY(end_call(ctx, sl));
      m.phase = 2;
      return LB_OK;
    }
  }
  // the package's worker bookkeeping (index.ts:557-568): jobs retried set by set,
  // sets verified by a passing aggregate (after phase 2's own merged-check stats)
  sl.h_stats[0] = m.retried_jobs;
  sl.h_stats[1] = m.fast_sets;
  if (m.agg) {
    memcpy(m.out_job_sig96, sm_h<uint8_t>(sl, L.h_agg96), (size_t)nj * 96);
    memcpy(m.out_job_count, sm_h<uint8_t>(sl, L.h_aggcnt), (size_t)nj * 4);
  }
  m.active = false;
  m.phase = 0;
  return LB_OK;
}

// Launch the phase 2 of every same-message call whose phase 1 has completed
// (called from every async entry point and lb_wait: no blocking).
int sm_pump(lb_ctx* ctx) {
  for (int s = 0; s <= ctx->plan.n_slots; s++) {
    Slot& sl = ctx->slots[s];
    // (another call's failure is not this caller's: it stays on that slot's ticket)
    if (sl.busy && sl.sm.active && sl.sm.phase == 1) (void)sm_advance(ctx, sl, false);
  }
  return LB_OK;
}

}  // namespace

extern "C" {

int lb_verify_same_message_batch_async(lb_ctx* ctx, const lb_same_message_batch* b, uint8_t* out_valid,
                                       uint8_t* out_job_fast, uint64_t* out_ticket) {
  if (!ctx || !b || !out_ticket || (b->n_sets && !out_valid)) return LB_ERR_INVALID_ARGUMENT;
  LB_TRY(sm_validate(ctx, b));
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(sm_pump(ctx));
  Slot& sl = next_async_slot(ctx);
  LB_TRY(finish_slot(ctx, sl));
  pick_streams(ctx, sl);
  if (b->n_jobs == 0) {  // nothing to verify: a call that completes at once
    LB_TRY(begin_call(ctx, sl));
    LB_TRY(end_call_async(ctx, sl));
    *out_ticket = sl.ticket;
    return LB_OK;
  }
  borrow_idle_stream(ctx, sl);
  LB_TRY(sm_submit(ctx, sl, b, out_valid, out_job_fast));
  *out_ticket = sl.ticket;
  return LB_OK;
}

// Synchronous form: slot 0 as the two-stream DAG (lowest latency).
int lb_verify_same_message_batch(lb_ctx* ctx, const lb_same_message_batch* b, uint8_t* out_valid,
                                 uint8_t* out_job_fast, lb_verify_stats* stats) {
  if (!ctx || !b || (b->n_sets && !out_valid)) return LB_ERR_INVALID_ARGUMENT;
  if (stats) *stats = lb_verify_stats{0, 0, 0.0};
  if (b->n_jobs == 0) return LB_OK;
  LB_TRY(sm_validate(ctx, b));
  LB_HIP(hipSetDevice(ctx->device));
  BorrowGuard g{ctx};
  LB_TRY(borrow_second_stream(ctx, g));
  Slot& sl = ctx->slots[0];
  LB_TRY(finish_slot(ctx, sl));
  pick_streams(ctx, sl);
  LB_TRY(sm_submit(ctx, sl, b, out_valid, out_job_fast));
  const uint64_t t = sl.ticket;
  LB_TRY(finish_slot(ctx, sl));
  fill_stats(ctx, t, stats);
  return LB_OK;
}

// The same calls with each job's aggregate signature: the verdicts, fast flags and stats of
// lb_verify_same_message_batch[_async], plus the stage sm_job_sig on the slot's stream.
int lb_verify_same_message_batch_agg_async(lb_ctx* ctx, const lb_same_message_batch* b, const uint8_t* agg_mask,
                                           uint8_t* out_valid, uint8_t* out_job_fast, uint8_t* out_job_sig96,
                                           uint32_t* out_job_count, uint64_t* out_ticket) {
  if (!ctx || !b || !out_ticket || (b->n_sets && !out_valid) || (b->n_jobs && (!out_job_sig96 || !out_job_count)))
    return LB_ERR_INVALID_ARGUMENT;
  LB_TRY(sm_validate(ctx, b));
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(sm_pump(ctx));
  Slot& sl = next_async_slot(ctx);
  LB_TRY(finish_slot(ctx, sl));
  pick_streams(ctx, sl);
  if (b->n_jobs == 0) {  // nothing to verify: a call that completes at once
    LB_TRY(begin_call(ctx, sl));
    LB_TRY(end_call_async(ctx, sl));
    *out_ticket = sl.ticket;
    return LB_OK;
  }
  borrow_idle_stream(ctx, sl);
  const SmAggOut agg{agg_mask, out_job_sig96, out_job_count};
  LB_TRY(sm_submit(ctx, sl, b, out_valid, out_job_fast, &agg));
  *out_ticket = sl.ticket;
  return LB_OK;
}

int lb_verify_same_message_batch_agg(lb_ctx* ctx, const lb_same_message_batch* b, const uint8_t* agg_mask,
                                     uint8_t* out_valid, uint8_t* out_job_fast, uint8_t* out_job_sig96,
                                     uint32_t* out_job_count, lb_verify_stats* stats) {
  if (!ctx || !b || (b->n_sets && !out_valid) || (b->n_jobs && (!out_job_sig96 || !out_job_count)))
    return LB_ERR_INVALID_ARGUMENT;
  if (stats) *stats = lb_verify_stats{0, 0, 0.0};
  if (b->n_jobs == 0) return LB_OK;
  LB_TRY(sm_validate(ctx, b));
  LB_HIP(hipSetDevice(ctx->device));
  BorrowGuard g{ctx};
  LB_TRY(borrow_second_stream(ctx, g));
  Slot& sl = ctx->slots[0];
  LB_TRY(finish_slot(ctx, sl));
  pick_streams(ctx, sl);
  const SmAggOut agg{agg_mask, out_job_sig96, out_job_count};
  LB_TRY(sm_submit(ctx, sl, b, out_valid, out_job_fast, &agg));
  const uint64_t t = sl.ticket;
  LB_TRY(finish_slot(ctx, sl));
  fill_stats(ctx, t, stats);
  return LB_OK;
}

// Signature.aggregate over many groups at once (the pools' aggregation without a verification):
// every signature decoded once (validate=true, or LB_AGG_NO_CHECK: signatureFromBytesNoCheck),
// then k_job_sig with "loaded" as the include flag, on the idle helper slot.
int lb_aggregate_signature_groups(lb_ctx* ctx, uint32_t n_groups, const uint32_t* group_offsets,
                                  const uint8_t* signatures, const uint32_t* sig_offsets, uint32_t flags,
                                  uint8_t* out96, int32_t* out_bad_index) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  if (n_groups == 0) return LB_OK;
  if (!group_offsets || !signatures || !sig_offsets || !out96 || !out_bad_index || (flags & ~LB_AGG_NO_CHECK)) {
    ctx->err = "lb_aggregate_signature_groups: null pointer or unknown flag";
    return LB_ERR_INVALID_ARGUMENT;
  }
  if (group_offsets[0] != 0) {
    ctx->err = "group_offsets must start at 0";
    return LB_ERR_INVALID_ARGUMENT;
  }
  for (uint32_t g = 0; g < n_groups; g++)
    if (group_offsets[g + 1] <= group_offsets[g]) {
      ctx->err = group_offsets[g + 1] == group_offsets[g] ? "EMPTY_AGGREGATE_ARRAY" : "group_offsets not monotone";
      return LB_ERR_INVALID_ARGUMENT;
    }
  const uint32_t n = group_offsets[n_groups];
  if (sig_offsets[0] != 0) return LB_ERR_INVALID_ARGUMENT;
  for (uint32_t i = 0; i < n; i++)
    if (sig_offsets[i + 1] < sig_offsets[i]) return LB_ERR_INVALID_ARGUMENT;
  std::vector<uint8_t> st(n);
  HelperCall c(ctx);
  auto d_s = c.in(signatures, sig_offsets[n]);
  auto d_o = c.in(sig_offsets, (size_t)n + 1);
  auto d_g = c.in(group_offsets, (size_t)n_groups + 1);
  auto d_sig = c.scratch<g2j>(n);
  auto d_st = c.out(st.data(), n);
  auto d_inc = c.scratch<uint8_t>(n);
  auto d_out = c.out(out96, (size_t)n_groups * 96);
  auto d_cnt = c.scratch<uint32_t>(n_groups);
  LB_TRY(c.begin());
  if (flags & LB_AGG_NO_CHECK)
    LB_LAUNCH(k_decode_sigs_nocheck, blocks_for(n), TPB, n, d_s, d_o, d_sig, d_st);
  else
    LB_LAUNCH(k_decode_sigs, blocks_for(n), TPB, n, d_s, d_o, (const uint8_t*)nullptr, d_sig, d_st);
  LB_LAUNCH(k_inc_status, blocks_for(n, 256), 256u, n, (const uint8_t*)d_st, d_inc);
  const uint32_t jpw = job_sig_jobs_per_wg(n_groups, n);
  const uint32_t runs = (n_groups + jpw - 1) / jpw;
  LB_LAUNCH(k_job_sig, runs < 16384u ? runs : 16384u, TPB, n_groups, jpw, d_g, (const g2j*)d_sig, (const uint8_t*)d_inc,
            d_out, d_cnt);
  LB_TRY(c.end());
  for (uint32_t g = 0; g < n_groups; g++) {
    out_bad_index[g] = -1;
    for (uint32_t i = group_offsets[g]; i < group_offsets[g + 1]; i++)
      if (st[i] != LB_ST_OK) {
        out_bad_index[g] = (int32_t)i;
        memset(out96 + (size_t)g * 96, 0, 96);
        break;
      }
  }
  return LB_OK;
}

int lb_verify_same_message(lb_ctx* ctx, uint32_t n, const uint8_t* pks, const uint8_t* sigs, const uint32_t* sig_off,
                           const uint8_t* message, const uint8_t* seed, uint8_t* out_valid,
                           uint32_t* out_used_fast_path) {
  if (!ctx || (n && (!pks || !sigs || !sig_off || !message || !seed || !out_valid))) return LB_ERR_INVALID_ARGUMENT;
  if (out_used_fast_path) *out_used_fast_path = 0;
  if (n == 0) return LB_OK;
  const uint32_t job_off[2] = {0, n};
  lb_same_message_batch b{};
  b.n_jobs = 1;
  b.n_sets = n;
  b.job_offsets = job_off;
  b.pubkeys = pks;
  b.signatures = sigs;
  b.sig_offsets = sig_off;
  b.messages = message;
  b.seed = seed;
  uint8_t fast = 0;
  LB_TRY(lb_verify_same_message_batch(ctx, &b, out_valid, &fast, nullptr));
  if (out_used_fast_path) *out_used_fast_path = fast;
  return LB_OK;
}

int lb_set_same_message_mode(lb_ctx* ctx, uint32_t mode) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  if (mode != LB_SM_PLAIN && mode != LB_SM_RANDOMIZED) {
    ctx->err = "lb_set_same_message_mode: LB_SM_PLAIN or LB_SM_RANDOMIZED";
    return LB_ERR_INVALID_ARGUMENT;
  }
  ctx->sm_mode = mode;
  return LB_OK;
}

int lb_same_message_mode(const lb_ctx* ctx) { return ctx ? (int)ctx->sm_mode : LB_ERR_INVALID_ARGUMENT; }

// Stage-level: the front of phase 1 alone (decode + aggregation in the context's mode) on the
// idle slot 0, the jobs' aggregated sets copied out.
int lb_same_message_aggregates(lb_ctx* ctx, const lb_same_message_batch* b, uint8_t* out_pk96, uint8_t* out_sig192,
                               uint8_t* out_job_bad) {
  if (!ctx || !b || (b->n_jobs && (!out_pk96 || !out_sig192 || !out_job_bad))) return LB_ERR_INVALID_ARGUMENT;
  if (b->n_jobs == 0) return LB_OK;
  LB_TRY(sm_validate(ctx, b));
  LB_HIP(hipSetDevice(ctx->device));
  LB_TRY(helper_slot(ctx));
  Slot& sl = ctx->slots[0];
  const uint32_t nj = b->n_jobs;
  SmShape shape;
  SmLayout L;
  LB_TRY(sm_prepare(ctx, sl, b, false, true, shape, L));
  LB_TRY(sm_front(ctx, sl, b, ctx->sm_mode, shape, L));
  const uint8_t *h_jbad = sm_h<const uint8_t>(sl, L.h_jbad), *h_jpkst = sm_h<const uint8_t>(sl, L.h_jpkst);
  LB_HIP(hipMemcpyAsync(sm_h<uint8_t>(sl, L.h_jbad), sm_d<uint8_t>(sl, L.d_jbad), nj, hipMemcpyDeviceToHost, sl.st[0]));
  LB_HIP(hipMemcpyAsync(sm_h<uint8_t>(sl, L.h_jpkst), sm_d<uint8_t>(sl, L.d_jpkst), nj, hipMemcpyDeviceToHost,
                        sl.st[0]));
  LB_HIP(hipMemcpyAsync(out_pk96, sm_d<uint8_t>(sl, L.d_pk96), (size_t)nj * 96, hipMemcpyDeviceToHost, sl.st[0]));
  LB_HIP(hipMemcpyAsync(out_sig192, sm_d<uint8_t>(sl, L.d_sig192), (size_t)nj * 192, hipMemcpyDeviceToHost, sl.st[0]));
  LB_HIP(hipStreamSynchronize(sl.st[0]));
  for (uint32_t j = 0; j < nj; j++) {
    const bool bad = h_jbad[j] || h_jpkst[j] != LB_ST_OK;
    out_job_bad[j] = bad ? 1 : 0;
    if (bad) {
      memset(out_pk96 + (size_t)j * 96, 0, 96);
      memset(out_sig192 + (size_t)j * 192, 0, 192);
    }
  }
  return LB_OK;
}

int lb_pairing(lb_ctx* ctx, uint32_t n, const uint8_t* g1_96, const uint8_t* g2_192, uint8_t* out576) {
  if (!ctx || (n && (!g1_96 || !g2_192 || !out576))) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  HelperCall c(ctx);
  auto d1 = c.in(g1_96, (size_t)n * 96);
  auto d2 = c.in(g2_192, (size_t)n * 192);
  auto d_out = c.out(out576, (size_t)n * 576);
  LB_TRY(c.begin());
  LB_LAUNCH(k_pairing, blocks_for(n), TPB, n, d1, d2, d_out);
  return c.end();
}

int lb_batch_scalars(lb_ctx* ctx, const uint8_t* seed, uint32_t first, uint32_t n, uint64_t* out) {
  if (!ctx || !seed || (n && !out)) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  HelperCall c(ctx);
  auto d_seed = c.in(seed, 32);
  auto d_out = c.out(out, n);
  LB_TRY(c.begin());
  LB_LAUNCH(k_scalars, blocks_for(n), TPB, d_seed, first, n, d_out);
  return c.end();
}

// [k_i] P_i for n points of `bytes` uncompressed bytes each (kernel: k_g1_mul / k_g2_mul)
static int point_mul(lb_ctx* ctx, uint32_t n, size_t bytes, const uint8_t* in, const uint64_t* k, uint8_t* out,
                     void (*kernel)(uint32_t, const uint8_t*, const uint64_t*, uint8_t*)) {
  if (!ctx || (n && (!in || !k || !out))) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  HelperCall c(ctx);
  auto d_in = c.in(in, (size_t)n * bytes);
  auto d_k = c.in(k, n);
  auto d_out = c.out(out, (size_t)n * bytes);
  LB_TRY(c.begin());
  LB_LAUNCH(kernel, blocks_for(n), TPB, n, (const uint8_t*)d_in, (const uint64_t*)d_k, (uint8_t*)d_out);
  return c.end();
}
int lb_g1_mul(lb_ctx* ctx, uint32_t n, const uint8_t* in96, const uint64_t* k, uint8_t* out96) {
  return point_mul(ctx, n, 96, in96, k, out96, k_g1_mul);
}
int lb_g2_mul(lb_ctx* ctx, uint32_t n, const uint8_t* in192, const uint64_t* k, uint8_t* out192) {
  return point_mul(ctx, n, 192, in192, k, out192, k_g2_mul);
}

// sum_i (a_i + b_i lambda) P_i through the merged check's bucket MSM (k_msm.hip),
// a_i / b_i = the low / high 32 bits of raw[i]: the MSM alone, for tests.
int lb_g2_msm(lb_ctx* ctx, uint32_t n, const uint8_t* in192, const uint64_t* raw, uint8_t* out192) {
  if (!ctx || !out192 || (n && (!in192 || !raw))) return LB_ERR_INVALID_ARGUMENT;
  if (n > (1u << 28)) {
    ctx->err = "lb_g2_msm: too many points";
    return LB_ERR_INVALID_ARGUMENT;
  }
  const uint32_t ns = n ? n : 1;
  const size_t n_ent = 2 * (size_t)ns * LB_MSM_W, max_chunks = n_ent / LB_MSM_T + LB_MSM_BUCKETS;
  const uint32_t req[2] = {0, n};
  HelperCall c(ctx);
  auto d_in = c.in(in192, (size_t)n * 192, n != 0);
  auto d_raw = c.in(raw, n, n != 0);
  auto d_req = c.in(req, 2);
  auto d_pts = c.scratch<g2j>(ns);
  auto d_st = c.scratch<uint8_t>(ns);
  auto d_keys = c.scratch<uint32_t>(n_ent);
  auto d_sorted = c.scratch<uint32_t>(n_ent);
  auto d_hist = c.scratch<uint32_t>(4 * (LB_MSM_BUCKETS + 1));
  auto d_csum = c.scratch<g2j>(max_chunks);
  auto d_bsum = c.scratch<g2j>(LB_MSM_BUCKETS);
  auto d_G = c.scratch<g2j>(LB_MSM_POS);
  auto d_S = c.scratch<g2a>(1);
  auto d_out = c.out(out192, 192);
  LB_TRY(c.begin());
  uint32_t* d_off = d_hist + (LB_MSM_BUCKETS + 1);
  uint32_t* d_coff = d_off + (LB_MSM_BUCKETS + 1);
  uint32_t* d_cur = d_coff + (LB_MSM_BUCKETS + 1);
  LB_HIP(hipMemsetAsync(d_hist, 0, (LB_MSM_BUCKETS + 1) * sizeof(uint32_t), ctx->stream));
  if (n) {
    LB_LAUNCH(k_msm_load, blocks_for(n), TPB, n, (const uint8_t*)d_in, d_pts, d_st);
    LB_LAUNCH(k_msm_scalars, 1u, TPB, 1u, (const uint32_t*)d_req, (const uint8_t*)nullptr, (const uint64_t*)d_raw,
              (const g2j*)d_pts, (const uint8_t*)d_st, (const uint8_t*)nullptr, d_keys, d_hist);
  }
  LB_LAUNCH(k_msm_scan, 1u, 1024u, (const uint32_t*)d_hist, d_off, d_coff, d_cur, LB_MSM_T);
  if (n) LB_LAUNCH(k_msm_scatter, blocks_for((uint32_t)n_ent, 256), 256u, (uint32_t)n_ent, (const uint32_t*)d_keys,
                   (const uint32_t*)d_off, d_cur, d_sorted);
  LB_LAUNCH(k_msm_chunks, blocks_for((uint32_t)max_chunks), TPB, (uint32_t)max_chunks, (const uint32_t*)d_off,
            (const uint32_t*)d_coff, (const uint32_t*)d_sorted, (const g2j*)d_pts, d_csum, LB_MSM_T);
  LB_LAUNCH(k_msm_buckets, blocks_for(LB_MSM_BUCKETS * LB_MSM_BLANES), TPB, (const uint32_t*)d_coff,
            (const g2j*)d_csum, d_bsum, LB_MSM_BLANES);
  LB_LAUNCH(k_msm_bits<LB_MSM_BITS_TPB>, LB_MSM_POS, LB_MSM_BITS_TPB, (const g2j*)d_bsum, d_G);
  LB_LAUNCH(k_msm_final, 1u, TPB, (const g2j*)d_G, d_S);
  LB_LAUNCH(k_g2a_serialize, 1u, TPB, 1u, (const g2a*)d_S, d_out);
  return c.end();
}

// A timing event that lives as long as its scope
struct ScopedEvent {
  hipEvent_t e = nullptr;
  ~ScopedEvent() {
    if (e) (void)hipEventDestroy(e);
  }
};

// Round program on n instances, one workgroup each (tests, timing): prog_words
// == nullptr runs the embedded program `prog` (LB_LP_PROG_*), else the caller's
// encoded program (lodestar_amd/lpgen) of n_words words.  in16: n x n_in records
// of 16 words (canonical Montgomery limbs), in_flags: n x n_inflag words; out16:
// n x n_out records, out_flags: n x n_outflag words; *out_ms: kernel time;
// stamps (optional): s_memtime after each round of instance 0.
int lb_lp_program_run(lb_ctx* ctx, uint32_t prog, const uint32_t* prog_words, size_t n_words, uint32_t n,
                      const uint32_t* in16, const uint32_t* in_flags, uint32_t* out16, uint32_t* out_flags,
                      float* out_ms, uint64_t* stamps) {
  if (!ctx || n == 0 || !in16 || !out16) return LB_ERR_INVALID_ARGUMENT;
  if (!prog_words && prog >= LB_LP_NPROGS) return LB_ERR_INVALID_ARGUMENT;
  // (the wide merged-check programs are compiled for k_lp_mtail's LB_LP_MTAIL_ROWS rows, more
  // than k_lp_program's workgroup runs)
  if (!prog_words && LB_LP_MTAIL_ROWS > LB_LP_ROWS &&
      (prog == LB_LP_PROG_MTAIL_CHECK_WIDE || prog == LB_LP_PROG_MTAIL_PARTIAL_WIDE))
    return LB_ERR_INVALID_ARGUMENT;
  if (prog_words && (n_words < LB_LP_HDR || prog_words[0] != 0x4C500004u)) return LB_ERR_INVALID_ARGUMENT;
  const uint32_t* hw = prog_words ? prog_words : lb_lp_blob + LB_LP_PROGS[prog].off;
  const uint32_t n_rounds = hw[1], n_in = hw[5], n_inflag = hw[6], n_out = hw[7], n_outflag = hw[8];
  if ((n_inflag && !in_flags) || (n_outflag && !out_flags)) return LB_ERR_INVALID_ARGUMENT;
  // (the flag buffers hold one word more than the host's arrays, the stamps one round more)
  const size_t fl_w = (size_t)n * n_inflag + 1, out_w = (size_t)n * n_out * 16, ofl_w = (size_t)n * n_outflag + 1;
  HelperCall c(ctx);
  auto d_words = c.in(prog_words, n_words, prog_words != nullptr);
  auto d_in = c.in(in16, (size_t)n * n_in * 16);
  auto d_fl = c.scratch<uint32_t>(fl_w);
  auto d_out = c.scratch<uint32_t>(out_w);
  auto d_ofl = c.scratch<uint32_t>(ofl_w);
  auto d_st = c.scratch<unsigned long long>((size_t)(n_rounds + 1) * LB_LP_STAMPS, stamps != nullptr);
  LB_TRY(c.begin());
  if (!prog_words) LB_TRY(lp_ensure(ctx));
  const uint32_t* d_prog = prog_words ? (const uint32_t*)d_words : ctx->d_lp.d + LB_LP_PROGS[prog].off;
  if (n_inflag) LB_HIP(hipMemcpyAsync(d_fl, in_flags, (fl_w - 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  ScopedEvent e0, e1;
  LB_HIP(hipEventCreate(&e0.e));
  LB_HIP(hipEventCreate(&e1.e));
  LB_HIP(hipEventRecord(e0.e, ctx->stream));
  LB_LAUNCH(k_lp_program, n, LB_LP_TPB, d_prog, n, d_in, n_in * 16u, (const uint32_t*)d_fl, n_inflag, d_out,
            n_out * 16u, d_ofl, n_outflag, d_st);
  LB_HIP(hipEventRecord(e1.e, ctx->stream));
  LB_HIP(hipMemcpyAsync(out16, d_out, out_w * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (n_outflag) LB_HIP(hipMemcpyAsync(out_flags, d_ofl, (ofl_w - 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (stamps)
    LB_HIP(hipMemcpyAsync(stamps, d_st, (size_t)n_rounds * LB_LP_STAMPS * 8, hipMemcpyDeviceToHost, ctx->stream));
  LB_TRY(c.end());
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0.e, e1.e);
  if (out_ms) *out_ms = ms;
  return LB_OK;
}

int lb_set_latency_path(lb_ctx* ctx, uint32_t max_sets) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  // (k_lp_verify's product tree has LB_LP_TREE_LEVELS levels of arrival counters: a
  // request longer than 2^levels sets would count past them)
  ctx->cfg.lp_max_sets = max_sets < (1u << LB_LP_TREE_LEVELS) ? max_sets : (1u << LB_LP_TREE_LEVELS);
  ctx->cfg.lp_explicit = true;
  return LB_OK;
}

int lb_sk_to_pk(lb_ctx* ctx, uint32_t n, const uint8_t* sk32, uint8_t* out96) {
  if (!ctx || (n && (!sk32 || !out96))) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  HelperCall c(ctx);
  auto d_k = c.in(sk32, (size_t)n * 32);
  auto d_out = c.out(out96, (size_t)n * 96);
  LB_TRY(c.begin());
  LB_LAUNCH(k_sk_to_pk, blocks_for(n), TPB, n, d_k, d_out);
  return c.end();
}

int lb_sign(lb_ctx* ctx, uint32_t n, const uint8_t* sk32, const uint8_t* messages, uint8_t* out96) {
  if (!ctx || (n && (!sk32 || !messages || !out96))) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  HelperCall c(ctx);
  auto d_k = c.in(sk32, (size_t)n * 32);
  auto d_m = c.in(messages, (size_t)n * 32);
  auto d_out = c.out(out96, (size_t)n * 96);
  LB_TRY(c.begin());
  LB_LAUNCH(k_sign, blocks_for(n), TPB, n, d_k, d_m, d_out);
  return c.end();
}

}  // extern "C"

// ============================================================================
// Blob KZG proof verification (k_kzg.hip)
// ============================================================================
namespace {

// What persists across the KZG calls, on first use: the setup's pair of slots and the roots
// table.  After the call's begin(), which has retired the calls in flight.
int kzg_ensure(lb_ctx* ctx) {
  KzgState& k = ctx->kzg;
  LB_TRY(k.neg_tau.reserve(ctx, 2, 0));
  if (k.roots.n) return LB_OK;
  LB_TRY(k.roots.reserve(ctx, LB_KZG_N, 0));
  LB_LAUNCH(k_kzg_roots, LB_KZG_N / 256, 256, k.roots.d);
  LB_HIP(hipStreamSynchronize(ctx->stream));
  k.roots.n = LB_KZG_N;  // (built)
  return LB_OK;
}

// device buffers of a verify call's pairing tail, as the call declared them
struct KzgBufs {
  CarvePtr<const uint8_t> com, proofs, z, y;
  CarvePtr<uint8_t> status, pt_status, skip, scalars, verdict;
  CarvePtr<g1j> P, lad, AB;
  CarvePtr<fp12> f;
};

// The tail's own buffers for n items, behind the commitments, proofs, z, y and statuses the
// call has declared; `verdicts` (n bytes) is where end() leaves them
KzgBufs kzg_declare_tail(HelperCall& c, uint32_t n, CarvePtr<const uint8_t> com, CarvePtr<const uint8_t> proofs,
                         CarvePtr<const uint8_t> z, CarvePtr<const uint8_t> y, CarvePtr<uint8_t> status,
                         uint8_t* verdicts) {
  const size_t m = n;
  KzgBufs b{com, proofs, z, y, status};
  b.pt_status = c.scratch<uint8_t>(2 * m);
  b.skip = c.scratch<uint8_t>(16);
  b.scalars = c.scratch<uint8_t>((3 * m + 1) * 32);
  b.verdict = c.out(verdicts, m);
  b.P = c.scratch<g1j>(2 * m + 1);
  b.lad = c.scratch<g1j>(3 * m + 1);
  b.AB = c.scratch<g1j>(2 * m);
  b.f = c.scratch<fp12>(2 * m);
  return b;
}

// The pairing tail on device-resident commitments, proofs, z and y: decode, statuses and
// scalars, ladders, sums, two Miller loops per check, final exponentiation.  Batch mode
// leaves one verdict, each mode one per item (the points decoded by a batch pass are reused).
int kzg_tail(lb_ctx* ctx, const KzgBufs& b, uint32_t n, uint32_t mode) {
  const KzgState& k = ctx->kzg;
  if (mode == LB_KZG_BATCH)
    LB_LAUNCH(k_kzg_decode, blocks_for(2 * n + 1), TPB, n, (const uint8_t*)b.com, (const uint8_t*)b.proofs, b.P,
              b.pt_status);
  LB_LAUNCH(k_kzg_rho, 1u, TPB, n, mode, (const uint8_t*)b.com, (const uint8_t*)b.proofs, (const uint8_t*)b.z,
            (const uint8_t*)b.y, (const uint8_t*)b.pt_status, b.status, b.scalars, b.skip);
  const uint32_t jobs = mode == LB_KZG_BATCH ? 3 * n + 1 : 2 * n;
  LB_LAUNCH(k_kzg_ladder, blocks_for(jobs), TPB, n, mode, (const g1j*)b.P, (const uint8_t*)b.scalars,
            (const uint8_t*)b.skip, b.lad);
  uint32_t m = 1;
  if (mode == LB_KZG_BATCH) {
    // A = sum rho_i pi_i, B = sum of the other 2n + 1 ladders (a skipped batch sums stale
    // points that nothing reads: k_kzg_miller and k_kzg_final skip too)
    LB_LAUNCH(k_jac_sum<fp>, 1u, 256u, n, (const g1j*)b.lad, b.AB);
    LB_LAUNCH(k_jac_sum<fp>, 1u, 256u, 2 * n + 1, (const g1j*)(b.lad + n), b.AB + 1);
  } else {
    m = n;
    LB_LAUNCH(k_kzg_each_sum, blocks_for(n), TPB, n, (const g1j*)b.P, (const g1j*)b.lad, b.AB);
  }
  LB_LAUNCH(k_kzg_miller, blocks_for(2 * m), TPB, m, (const g1j*)b.AB, (const g2a*)k.neg_tau.d,
            mode == LB_KZG_BATCH ? (const uint8_t*)b.skip : (const uint8_t*)nullptr, b.f);
  LB_LAUNCH(k_kzg_final, blocks_for(m), TPB, m, mode, (const fp12*)b.f, (const uint8_t*)b.status,
            (const uint8_t*)b.skip, b.verdict);
  return LB_OK;
}

// What a verify call's two outputs come back into (kzg_declare_tail, kzg_finish_verify)
struct KzgVerdicts {
  uint8_t st[LB_KZG_MAX_BLOBS], v[LB_KZG_MAX_BLOBS];
};

// verdicts of a verify call once its tail is enqueued: statuses, the batch verdict ([0] of the
// verdicts a batch pass leaves) and, for a failed batch with out_each, every item's own check:
// the per-item tail on the buffers still bound, and end() once more for its verdicts
int kzg_finish_verify(HelperCall& c, const KzgBufs& b, KzgVerdicts& r, uint32_t n, int32_t* out_ok,
                      uint8_t* out_status, uint8_t* out_each) {
  lb_ctx* ctx = c.ctx;
  LB_TRY(c.end());
  bool ok = r.v[0] == 1;
  for (uint32_t i = 0; i < n; i++) ok = ok && r.st[i] == LB_KZG_OK;
  *out_ok = ok ? 1 : 0;
  if (out_status) memcpy(out_status, r.st, n);
  if (out_each) {
    if (ok) {
      memset(out_each, 1, n);
    } else {
      LB_TRY(kzg_tail(ctx, b, n, LB_KZG_EACH));
      LB_TRY(c.end());
      for (uint32_t i = 0; i < n; i++) out_each[i] = (r.st[i] == LB_KZG_OK && r.v[i] == 1) ? 1 : 0;
    }
  }
  return LB_OK;
}

int kzg_check_verify_args(lb_ctx* ctx, uint32_t n, bool ptrs_ok, const char* what) {
  if (n > LB_KZG_MAX_BLOBS) {
    ctx->err = std::string(what) + ": more than LB_KZG_MAX_BLOBS items";
    return LB_ERR_INVALID_ARGUMENT;
  }
  if (!ptrs_ok) {
    ctx->err = std::string(what) + ": null pointer";
    return LB_ERR_INVALID_ARGUMENT;
  }
  return LB_OK;
}

}  // namespace

extern "C" {

int lb_kzg_setup_loaded(const lb_ctx* ctx) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  return ctx->kzg.loaded ? 1 : 0;
}

int lb_kzg_load_setup(lb_ctx* ctx, const uint8_t* g2_tau96) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  if (!g2_tau96) {
    ctx->err = "lb_kzg_load_setup: null pointer";
    return LB_ERR_INVALID_ARGUMENT;
  }
  uint8_t st = 0xff;
  HelperCall c(ctx);
  auto d_tau = c.in(g2_tau96, 96);
  auto d_st = c.out(&st, 1);
  LB_TRY(c.begin());
  LB_TRY(kzg_ensure(ctx));
  KzgState& k = ctx->kzg;
  // the candidate is checked into slot [1] and copied over the loaded setup only when accepted
  LB_LAUNCH(k_kzg_setup_g2, 1u, TPB, d_tau, k.neg_tau.d + 1, d_st);
  LB_TRY(c.end());
  if (st != LB_ST_OK) {
    ctx->err = std::string("lb_kzg_load_setup: KZG_SETUP_G2_MONOMIAL[1] ") +
               (st == LB_ST_PK_INFINITY ? "is the point at infinity"
                : st == LB_ST_NOT_IN_GROUP ? "is not in G2"
                : st == LB_ST_NOT_ON_CURVE ? "is not on the curve"
                                           : "does not decode");
    return LB_ERR_INVALID_ARGUMENT;
  }
  LB_HIP(hipMemcpyAsync(k.neg_tau.d, k.neg_tau.d + 1, sizeof(g2a), hipMemcpyDeviceToDevice, ctx->stream));
  LB_HIP(hipStreamSynchronize(ctx->stream));
  k.loaded = true;
  return LB_OK;
}

int lb_kzg_blob_challenges(lb_ctx* ctx, uint32_t n, const uint8_t* blobs, const uint8_t* commitments48,
                           uint8_t* out_z32, uint8_t* out_y32, uint8_t* out_status) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  LB_TRY(kzg_check_verify_args(ctx, n, blobs && commitments48 && out_z32 && out_y32 && out_status,
                               "lb_kzg_blob_challenges"));
  HelperCall c(ctx);
  auto d_blobs = c.in(blobs, (size_t)n * LB_KZG_BLOB_BYTES);
  auto d_com = c.in(commitments48, (size_t)n * 48);
  auto d_z = c.out(out_z32, (size_t)n * 32);
  auto d_y = c.out(out_y32, (size_t)n * 32);
  auto d_st = c.out(out_status, n);
  LB_TRY(c.begin());
  LB_TRY(kzg_ensure(ctx));
  LB_TRY(c.stage("kzg_hash"));
  LB_LAUNCH(k_kzg_hash, n, LB_KZG_HASH_TPB, d_blobs, d_com, d_z, d_st);
  LB_TRY(c.stage("kzg_eval"));
  LB_LAUNCH(k_kzg_eval, n, LB_KZG_EVAL_TPB, d_blobs, (const fr*)ctx->kzg.roots.d, (const uint8_t*)d_z, d_y, d_st);
  return c.end();
}

int lb_kzg_evaluate(lb_ctx* ctx, uint32_t n, const uint8_t* blobs, const uint8_t* z32, uint8_t* out_y32,
                    uint8_t* out_status) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  LB_TRY(kzg_check_verify_args(ctx, n, blobs && z32 && out_y32 && out_status, "lb_kzg_evaluate"));
  HelperCall c(ctx);
  auto d_blobs = c.in(blobs, (size_t)n * LB_KZG_BLOB_BYTES);
  auto d_z = c.in(z32, (size_t)n * 32);
  auto d_y = c.out(out_y32, (size_t)n * 32);
  auto d_st = c.out(out_status, n);
  LB_TRY(c.begin());
  LB_TRY(kzg_ensure(ctx));
  LB_HIP(hipMemsetAsync(d_st, 0, n, ctx->stream));
  LB_TRY(c.stage("kzg_eval"));
  LB_LAUNCH(k_kzg_eval, n, LB_KZG_EVAL_TPB, d_blobs, (const fr*)ctx->kzg.roots.d, d_z, d_y, d_st);
  return c.end();
}

int lb_kzg_verify_blob_proof_batch(lb_ctx* ctx, uint32_t n, const uint8_t* blobs, const uint8_t* commitments48,
                                   const uint8_t* proofs48, int32_t* out_ok, uint8_t* out_status,
                                   uint8_t* out_each) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  LB_TRY(kzg_check_verify_args(ctx, n, out_ok && (n == 0 || (blobs && commitments48 && proofs48)),
                               "lb_kzg_verify_blob_proof_batch"));
  if (!ctx->kzg.loaded) {
    ctx->err = "lb_kzg_verify_blob_proof_batch: no trusted setup loaded (lb_kzg_load_setup)";
    return LB_ERR_INVALID_ARGUMENT;
  }
  if (n == 0) {
    *out_ok = 1;
    return LB_OK;
  }
  KzgVerdicts r;
  HelperCall c(ctx);
  auto d_blobs = c.in(blobs, (size_t)n * LB_KZG_BLOB_BYTES);
  auto d_com = c.in(commitments48, (size_t)n * 48);
  auto d_proofs = c.in(proofs48, (size_t)n * 48);
  auto d_z = c.scratch<uint8_t>((size_t)n * 32);
  auto d_y = c.scratch<uint8_t>((size_t)n * 32);
  auto d_st = c.out(r.st, n);
  const KzgBufs b = kzg_declare_tail(c, n, d_com, d_proofs, {d_z.off, d_z.base}, {d_y.off, d_y.base}, d_st, r.v);
  LB_TRY(c.begin());
  LB_TRY(kzg_ensure(ctx));
  LB_TRY(c.stage("kzg_hash"));
  LB_LAUNCH(k_kzg_hash, n, LB_KZG_HASH_TPB, d_blobs, d_com, d_z, d_st);
  LB_TRY(c.stage("kzg_eval"));
  LB_LAUNCH(k_kzg_eval, n, LB_KZG_EVAL_TPB, d_blobs, (const fr*)ctx->kzg.roots.d, (const uint8_t*)d_z, d_y, d_st);
  LB_TRY(c.stage("kzg_tail"));
  LB_TRY(kzg_tail(ctx, b, n, LB_KZG_BATCH));
  return kzg_finish_verify(c, b, r, n, out_ok, out_status, out_each);
}

int lb_kzg_verify_proof_batch(lb_ctx* ctx, uint32_t n, const uint8_t* commitments48, const uint8_t* z32,
                              const uint8_t* y32, const uint8_t* proofs48, int32_t* out_ok, uint8_t* out_status,
                              uint8_t* out_each) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  LB_TRY(kzg_check_verify_args(ctx, n, out_ok && (n == 0 || (commitments48 && z32 && y32 && proofs48)),
                               "lb_kzg_verify_proof_batch"));
  if (!ctx->kzg.loaded) {
    ctx->err = "lb_kzg_verify_proof_batch: no trusted setup loaded (lb_kzg_load_setup)";
    return LB_ERR_INVALID_ARGUMENT;
  }
  if (n == 0) {
    *out_ok = 1;
    return LB_OK;
  }
  KzgVerdicts r;
  HelperCall c(ctx);
  auto d_com = c.in(commitments48, (size_t)n * 48);
  auto d_proofs = c.in(proofs48, (size_t)n * 48);
  auto d_z = c.in(z32, (size_t)n * 32);
  auto d_y = c.in(y32, (size_t)n * 32);
  auto d_st = c.out(r.st, n);
  const KzgBufs b = kzg_declare_tail(c, n, d_com, d_proofs, d_z, d_y, d_st, r.v);
  LB_TRY(c.begin());
  LB_TRY(kzg_ensure(ctx));
  LB_HIP(hipMemsetAsync(d_st, 0, n, ctx->stream));
  LB_TRY(c.stage("kzg_tail"));
  LB_TRY(kzg_tail(ctx, b, n, LB_KZG_BATCH));
  return kzg_finish_verify(c, b, r, n, out_ok, out_status, out_each);
}

}  // extern "C"

// ============================================================================
// Blob KZG commitments and proofs (k_kzg_msm.hip)
// ============================================================================
namespace {

// device buffers of the fixed-base MSM: one group of jobs at a time
struct KzgMsmBufs {
  CarvePtr<uint32_t> keys, sorted, hist, off, coff, cursor;
  CarvePtr<g1j> csum, bsum, G;
};

static_assert(sizeof(g1j) == SZ_G1J, "carve record size");

// The MSM's buffers for a call of n jobs: those of one group, the call's largest (kzg_msm)
KzgMsmBufs kzg_declare_msm(HelperCall& c, uint32_t n) {
  const size_t g = n < LB_KZG_MSM_GROUP ? n : LB_KZG_MSM_GROUP, NB = LB_KZG_MSM_NB;
  KzgMsmBufs m;
  m.keys = c.scratch<uint32_t>(g * LB_KZG_MSM_ENT);
  m.sorted = c.scratch<uint32_t>(g * LB_KZG_MSM_ENT);
  m.hist = c.scratch<uint32_t>(g * NB);
  m.off = c.scratch<uint32_t>(g * (NB + 1));
  m.coff = c.scratch<uint32_t>(g * (NB + 1));
  m.cursor = c.scratch<uint32_t>(g * NB);
  m.csum = c.scratch<g1j>(g * LB_KZG_MSM_MAXC);
  m.bsum = c.scratch<g1j>(g * NB);
  m.G = c.scratch<g1j>(g * 8);
  return m;
}

// out48[k] = sum_i scalars[k][i] L[i] for n device-resident jobs, in groups of LB_KZG_MSM_GROUP;
// a scalar >= r sets status[k] = bad_code (kept when set already); such a job's output is zero
int kzg_msm(lb_ctx* ctx, const KzgMsmBufs& m, uint32_t n, const uint8_t* scalars, uint8_t* status, uint8_t bad_code,
            uint8_t* out48) {
  const g1a* T = ctx->kzg.g1_tab[ctx->kzg.g1_cur].d;
  for (uint32_t j0 = 0; j0 < n; j0 += LB_KZG_MSM_GROUP) {
    const uint32_t g = n - j0 < LB_KZG_MSM_GROUP ? n - j0 : LB_KZG_MSM_GROUP;
    const uint8_t* sc = scalars + (size_t)j0 * LB_KZG_BLOB_BYTES;
    LB_HIP(hipMemsetAsync(m.hist, 0, sizeof(uint32_t) * g * LB_KZG_MSM_NB, ctx->stream));
    LB_LAUNCH(k_kzg_msm_digits, (dim3(LB_KZG_N / 256, g)), 256u, sc, status + j0, bad_code, m.keys, m.hist);
    LB_LAUNCH(k_kzg_msm_scan, g, LB_KZG_MSM_NB, (const uint32_t*)m.hist, m.off, m.coff, m.cursor);
    LB_LAUNCH(k_kzg_msm_scatter, (dim3(LB_KZG_MSM_ENT / (256 * LB_KZG_MSM_SCAT_PER), g)), 256u,
              (const uint32_t*)m.keys, (const uint32_t*)m.off, m.cursor, m.sorted);
    LB_LAUNCH(k_kzg_msm_chunks, (dim3(blocks_for(LB_KZG_MSM_MAXC), g)), TPB, (const uint32_t*)m.off,
              (const uint32_t*)m.coff, (const uint32_t*)m.sorted, T, m.csum);
    LB_LAUNCH(k_kzg_msm_buckets, (dim3(LB_KZG_MSM_NB, g)), TPB, (const uint32_t*)m.coff, (const g1j*)m.csum, m.bsum);
    LB_LAUNCH(k_kzg_msm_bits, (dim3(8, g)), TPB, (const g1j*)m.bsum, m.G);
    LB_LAUNCH(k_kzg_msm_final, blocks_for(g), TPB, g, (const g1j*)m.G, (const uint8_t*)(status + j0),
              out48 + (size_t)j0 * 48);
  }
  return LB_OK;
}

// the checks every commitment / proof entry point makes before it touches the device
int kzg_check_g1_args(lb_ctx* ctx, uint32_t n, bool ptrs_ok, const char* what) {
  LB_TRY(kzg_check_verify_args(ctx, n, ptrs_ok, what));
  if (!ctx->kzg.g1_loaded) {
    ctx->err = std::string(what) + ": no G1 setup loaded (lb_kzg_load_setup_g1)";
    return LB_ERR_INVALID_ARGUMENT;
  }
  return LB_OK;
}

// n jobs of 4096 scalars each up, their MSM, results and statuses down
int kzg_lincomb(lb_ctx* ctx, uint32_t n, const uint8_t* scalars32, uint8_t bad_code, uint8_t* out48,
                uint8_t* out_status) {
  HelperCall c(ctx);
  auto d_sc = c.in(scalars32, (size_t)n * LB_KZG_BLOB_BYTES);
  auto d_st = c.out(out_status, n);
  auto d_out = c.out(out48, (size_t)n * 48);
  const KzgMsmBufs m = kzg_declare_msm(c, n);
  LB_TRY(c.begin());
  LB_TRY(kzg_ensure(ctx));
  LB_HIP(hipMemsetAsync(d_st, 0, n, ctx->stream));
  LB_TRY(c.stage("kzg_msm"));
  LB_TRY(kzg_msm(ctx, m, n, d_sc, d_st, bad_code, d_out));
  return c.end();
}

// blobs (and commitments or z) up; then the quotients' MSM.  with_hash: z from the transcript
// (compute_blob_kzg_proof), else z is given (compute_kzg_proof).
int kzg_prove(lb_ctx* ctx, uint32_t n, const uint8_t* blobs, const uint8_t* com48, const uint8_t* z32,
              uint8_t* out_proofs48, uint8_t* out_y32, uint8_t* out_status) {
  HelperCall c(ctx);
  auto d_blobs = c.in(blobs, (size_t)n * LB_KZG_BLOB_BYTES);
  auto d_com = c.in(com48, (size_t)n * 48, com48 != nullptr);
  // z: the caller's, or the transcript's; y: kept on the device when the caller does not want it
  // (CARVE_OUT without a host pointer is scratch)
  auto d_z = c.add<uint8_t>(com48 ? CARVE_SCRATCH : CARVE_IN, (size_t)n * 32, true, z32, nullptr);
  auto d_y = c.out(out_y32, (size_t)n * 32);
  auto d_st = c.out(out_status, n);
  auto d_quot = c.scratch<uint8_t>((size_t)n * LB_KZG_BLOB_BYTES);
  auto d_out = c.out(out_proofs48, (size_t)n * 48);
  const KzgMsmBufs m = kzg_declare_msm(c, n);
  LB_TRY(c.begin());
  LB_TRY(kzg_ensure(ctx));
  const fr* roots = ctx->kzg.roots.d;
  if (com48) {
    LB_TRY(c.stage("kzg_hash"));
    LB_LAUNCH(k_kzg_hash, n, LB_KZG_HASH_TPB, d_blobs, d_com, d_z, d_st);
    LB_LAUNCH(k_kzg_check_com, blocks_for(n), TPB, n, d_com, d_st);
  } else {
    LB_HIP(hipMemsetAsync(d_st, 0, n, ctx->stream));
  }
  LB_TRY(c.stage("kzg_eval"));
  LB_LAUNCH(k_kzg_eval, n, LB_KZG_EVAL_TPB, d_blobs, roots, (const uint8_t*)d_z, d_y, d_st);
  LB_TRY(c.stage("kzg_quot"));
  LB_LAUNCH(k_kzg_quotient, n, LB_KZG_EVAL_TPB, d_blobs, roots, (const uint8_t*)d_z, (const uint8_t*)d_y,
            (const uint8_t*)d_st, d_quot);
  LB_TRY(c.stage("kzg_msm"));
  LB_TRY(kzg_msm(ctx, m, n, d_quot, d_st, LB_KZG_BAD_SCALAR, d_out));
  return c.end();
}

}  // namespace

extern "C" {

int lb_kzg_setup_g1_loaded(const lb_ctx* ctx) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  return ctx->kzg.g1_loaded ? 1 : 0;
}

int lb_kzg_load_setup_g1(lb_ctx* ctx, const uint8_t* g1_lagrange48, int32_t* out_bad_index) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  if (!g1_lagrange48) {
    ctx->err = "lb_kzg_load_setup_g1: null pointer";
    return LB_ERR_INVALID_ARGUMENT;
  }
  if (out_bad_index) *out_bad_index = -1;
  // the file's points, their statuses, the Jacobian multiples before the inversion
  std::vector<uint8_t> st(LB_KZG_N);
  HelperCall c(ctx);
  auto d_in48 = c.in(g1_lagrange48, (size_t)LB_KZG_N * 48);
  auto d_pt_st = c.out(st.data(), LB_KZG_N);
  auto d_J = c.scratch<g1j>(LB_KZG_MSM_ENT);
  LB_TRY(c.begin());
  LB_TRY(kzg_ensure(ctx));
  KzgState& k = ctx->kzg;
  // the candidate's table is built beside the loaded one and takes its place only when accepted
  const int cand = k.g1_cur ^ 1;
  for (DevArray<g1a>& t : k.g1_tab) LB_TRY(t.reserve(ctx, LB_KZG_MSM_ENT, 0));
  LB_TRY(c.stage("kzg_setup_g1"));
  LB_LAUNCH(k_kzg_setup_g1, blocks_for(LB_KZG_N), TPB, d_in48, d_J, k.g1_tab[cand].d, d_pt_st);
  LB_TRY(c.end());
  for (uint32_t i = 0; i < LB_KZG_N; i++) {
    if (st[i] == LB_ST_OK) continue;
    if (out_bad_index) *out_bad_index = (int32_t)i;
    ctx->n_stages = 0;  // (a refused load publishes no stage)
    ctx->err = "lb_kzg_load_setup_g1: G1 point " + std::to_string(i) + " of the file " +
               (st[i] == LB_ST_NOT_IN_GROUP ? "is not in G1"
                : st[i] == LB_ST_NOT_ON_CURVE ? "is not on the curve"
                                              : "does not decode");
    return LB_ERR_INVALID_ARGUMENT;
  }
  k.g1_cur = cand;
  k.g1_loaded = true;
  return LB_OK;
}

int lb_kzg_g1_lincomb(lb_ctx* ctx, uint32_t n_jobs, const uint8_t* scalars32, uint8_t* out48, uint8_t* out_status) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  if (n_jobs == 0) return LB_OK;
  LB_TRY(kzg_check_g1_args(ctx, n_jobs, scalars32 && out48 && out_status, "lb_kzg_g1_lincomb"));
  return kzg_lincomb(ctx, n_jobs, scalars32, LB_KZG_BAD_SCALAR, out48, out_status);
}

int lb_kzg_blob_commitments(lb_ctx* ctx, uint32_t n, const uint8_t* blobs, uint8_t* out_commitments48,
                            uint8_t* out_status) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  LB_TRY(kzg_check_g1_args(ctx, n, blobs && out_commitments48 && out_status, "lb_kzg_blob_commitments"));
  // a blob is its polynomial's 4096 scalars as the MSM reads them
  return kzg_lincomb(ctx, n, blobs, LB_KZG_BAD_BLOB, out_commitments48, out_status);
}

int lb_kzg_blob_proofs(lb_ctx* ctx, uint32_t n, const uint8_t* blobs, const uint8_t* commitments48,
                       uint8_t* out_proofs48, uint8_t* out_status) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  LB_TRY(kzg_check_g1_args(ctx, n, blobs && commitments48 && out_proofs48 && out_status, "lb_kzg_blob_proofs"));
  return kzg_prove(ctx, n, blobs, commitments48, nullptr, out_proofs48, nullptr, out_status);
}

int lb_kzg_compute_proofs(lb_ctx* ctx, uint32_t n, const uint8_t* blobs, const uint8_t* z32, uint8_t* out_proofs48,
                          uint8_t* out_y32, uint8_t* out_status) {
  if (!ctx) return LB_ERR_INVALID_ARGUMENT;
  if (n == 0) return LB_OK;
  LB_TRY(kzg_check_g1_args(ctx, n, blobs && z32 && out_proofs48 && out_y32 && out_status, "lb_kzg_compute_proofs"));
  return kzg_prove(ctx, n, blobs, nullptr, z32, out_proofs48, out_y32, out_status);
}

}  // extern "C"
