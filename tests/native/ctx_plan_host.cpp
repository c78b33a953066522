// Host build of lodestar_amd/csrc/bls_ctx_plan.h for tests/test_ctx_plan.py (ctypes), and with
// -DCTX_PLAN_HOST_MAIN a stand-alone program that walks the configuration grid itself (the
// build that runs under -fsanitize=address,undefined).
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "../../lodestar_amd/csrc/bls_ctx_plan.h"
#include "../../lodestar_amd/csrc/bls_plan.h"  // (its switch table: the census)

using namespace lb;

static std::map<std::string, std::string> g_env;
static const char* env_lookup(const char* name) {
  auto it = g_env.find(name);
  return it == g_env.end() ? nullptr : it->second.c_str();
}

#define CFG_FIELDS(X)                                                                                         \
  X(max_hw_queues) X(slots) X(slot0_streams) X(prio_cus) X(prio_spread) X(prio_dyn) X(prio_hold_ms)          \
  X(prio_dyn_slots) X(tail_prio) X(scratch_budget_gb) X(sm_lp_decode) X(sm_randomized) X(tp_pause)           \
  X(fault_rerun) X(gt_lp) X(prio_kcopy) X(dag) X(stage_events)

#define PLAN_FIELDS(X)                                                                                        \
  X(lane) X(n_slots) X(prio_cus) X(prio_dyn) X(prio_dyn_slots) X(prio_hold_ms) X(tail_stream) X(q_plain)     \
  X(q_high) X(q_masked) X(hw_queues) X(err)

extern "C" {

void cp_env_clear() { g_env.clear(); }
void cp_env_set(const char* name, const char* value) { g_env[name] = value; }

CtxConfig* cp_config_new(int from_env) {
  CtxConfig* c = new CtxConfig();
  if (from_env) ctx_config_from_env(*c, env_lookup);
  return c;
}
void cp_config_free(CtxConfig* c) { delete c; }
int cp_config_nfields() {
  int n = 0;
#define X(f) n++;
  CFG_FIELDS(X)
#undef X
  return n;
}
const char* cp_config_field(int i) {
  static const char* names[] = {
#define X(f) #f,
      CFG_FIELDS(X)
#undef X
  };
  return names[i];
}
double cp_config_get(const CtxConfig* c, const char* name) {
#define X(f) \
  if (!strcmp(name, #f)) return (double)c->f;
  CFG_FIELDS(X)
#undef X
  return -999;
}
int cp_env_nknobs() { return (int)(sizeof(kCtxEnvKnobs) / sizeof(kCtxEnvKnobs[0])); }
const char* cp_env_knob(int i) { return kCtxEnvKnobs[i].name; }

CtxPlan* cp_plan_new(const CtxConfig* c, int cus, unsigned lane_bytes, int lane, int live_plain, int live_high,
                     int live_masked) {
  DeviceFacts d;
  d.cus = cus;
  d.lane_bytes = lane_bytes;
  return new CtxPlan(plan_context(*c, d, lane != 0, QueueTally{live_plain, live_high, live_masked}));
}
void cp_plan_free(CtxPlan* p) { delete p; }
double cp_plan_get(const CtxPlan* p, const char* name) {
#define X(f) \
  if (!strcmp(name, #f)) return (double)p->f;
  PLAN_FIELDS(X)
#undef X
  return -999;
}
const char* cp_plan_msg(const CtxPlan* p) { return p->msg; }
int cp_plan_streams(const CtxPlan* p, int s) { return p->streams_per_slot[s]; }
int cp_plan_mask_slot(const CtxPlan* p, int s) { return p->mask_slot[s]; }
int cp_plan_mask_words(const CtxPlan* p) { return (int)p->cu_mask.size(); }
unsigned cp_plan_mask_word(const CtxPlan* p, int i) { return p->cu_mask[(size_t)i]; }
// what creation does for stream i of slot s: the full stream's kind | the masked one's << 4 | starts masked << 8
int cp_plan_stream(const CtxPlan* p, int s, int i) {
  const StreamPlan& e = p->st[s][i];
  return (int)e.full | (int)e.mask << 4 | (int)e.starts_masked() << 8;
}
int cp_pipe_nknobs() { return (int)(sizeof(kEnvKnobs) / sizeof(kEnvKnobs[0])); }
const char* cp_pipe_knob(int i) { return kEnvKnobs[i].name; }

}  // extern "C"

#ifdef CTX_PLAN_HOST_MAIN
static int fail(const char* what, int ci) {
  std::printf("FAIL %s config=%d:", what, ci);
  for (auto& kv : g_env) std::printf(" %s=%s", kv.first.c_str(), kv.second.c_str());
  std::puts("");
  return 1;
}

int main() {
  const int slots[] = {1, 2, 3, 4, 8, 16}, cus[] = {0, 64, 256};
  const char* slot0[] = {nullptr, "1", "2"};
  int ci = 0;
  for (int n : slots)
    for (int dyn = 0; dyn < 2; dyn++)
      for (int v : {1, 2, 3, n})
        for (int cu : cus)
          for (int tail = 0; tail < 2; tail++)
            for (const char* s0 : slot0)
              for (int lane = 0; lane < 2; lane++, ci++) {
                g_env.clear();
                g_env["GPU_MAX_HW_QUEUES"] = "16";
                g_env["LB_SLOTS"] = std::to_string(n);
                g_env["LB_PRIO_DYN"] = std::to_string(dyn);
                g_env["LB_PRIO_DYN_SLOTS"] = std::to_string(v);
                g_env["LB_TAIL_PRIO"] = std::to_string(tail);
                if (s0) g_env["LB_SLOT0_STREAMS"] = s0;
                CtxConfig c;
                ctx_config_from_env(c, env_lookup);
                DeviceFacts d;
                d.cus = cu;
                d.lane_bytes = 3328;
                const CtxPlan p = plan_context(c, d, lane, QueueTally{});
                if (p.n_slots != (lane ? 1 : n)) return fail("slots", ci);
                const bool mask = !p.cu_mask.empty();
                if (mask != (!lane && cu == 256) || (mask && p.cu_mask.size() != 8)) return fail("mask", ci);
                int plain = 0, high = 1 + tail, masked = 0;  // (lb_gt_check's aux stream, the tail stream)
                for (int s = 0; s <= p.n_slots; s++) {
                  if (p.st[s][0].full == ST_NONE && p.st[s][0].mask == ST_NONE) return fail("a slot without a stream", ci);
                  if (p.st[s][0].full == ST_ALIAS0 || p.st[s][0].mask == ST_ALIAS0) return fail("stream 0 an alias", ci);
                  if (s < p.n_slots && mask && !owned(p.st[p.mask_slot[s]][0].mask)) return fail("mask_slot", ci);
                  for (int i = 0; i < 2; i++) {
                    const StreamPlan& e = p.st[s][i];
                    if ((e.starts_masked() ? e.mask : e.full) == ST_NONE) return fail("st[] starts as nothing", ci);
                    plain += e.full == ST_OWN;
                    high += e.full == ST_HIGH;
                    masked += e.mask == ST_OWN;
                  }
                }
                if (plain != p.q_plain || high != p.q_high || masked != p.q_masked) return fail("tally", ci);
                // DESIGN.md §5.1's arithmetic, restated
                const bool dyn_on = dyn && mask;
                const int K = !mask ? 0 : dyn_on && v >= 1 && v < p.n_slots ? v : p.n_slots;
                int f_plain = 0, f_masked = 0;
                for (int s = 0; s < p.n_slots; s++) {
                  const int spp = s == 0 && s0 ? atoi(s0) : lane ? 1 : n <= 2 || (n == 3 && s == 0) ? 2 : 1;
                  if (spp != p.streams_per_slot[s]) return fail("streams per slot", ci);
                  if (!mask || dyn_on) f_plain += spp;
                  if (s < K) f_masked += dyn_on && K < p.n_slots ? 1 : spp;
                }
                if (f_plain != plain || f_masked != masked || high != 2 + tail) return fail("formula", ci);
                const int q = (plain < 16 ? plain : 16) + high + masked;
                if (q != p.hw_queues || (p.err != 0) != (q > 20) || (p.err && !p.msg[0])) return fail("guard", ci);
              }
  std::puts("ok");
  return 0;
}
#endif
