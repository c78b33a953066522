// Host build of lodestar_amd/csrc/bls_plan.h for tests/test_pipe_plan.py (ctypes), and with
// -DPLAN_HOST_MAIN a stand-alone program that walks the layout grid itself (the build that
// runs under -fsanitize=address,undefined).
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../lodestar_amd/csrc/bls_plan.h"

using namespace lb;

static std::map<std::string, std::string> g_env;
static const char* env_lookup(const char* name) {
  auto it = g_env.find(name);
  return it == g_env.end() ? nullptr : it->second.c_str();
}

#define CFG_FIELDS(X)                                                                                           \
  X(miller_mode) X(lines_min_sets) X(wave_max_sets) X(lines_waves) X(lines_waves_small) X(acc_lpr) X(acc_split) \
  X(acc_steps) X(step_mode) X(step_waves) X(tail_wave) X(merge_min_req) X(msm_min_sets) X(level_wc) X(msm_lanes) \
  X(wide_tail) X(msm_bits_lp) X(step_split) X(lp_decode) X(lp_hash_finish) X(msm_short) X(msm_short_max)         \
  X(msm_t_lone) X(lp_dec_max) X(lp_hf_max) X(lp_lines_max) X(lp_hash_full) X(lp_narrow) X(lp_lines)              \
  X(lp_max_sets) X(lp_lone_max) X(lp_explicit) X(mtail_lp) X(rtail_lp) X(tp_release) X(tp_release_cfg)

#define PLAN_FIELDS(X)                                                                                          \
  X(n_req) X(n_sets) X(ns) X(nr1) X(lone) X(partial) X(presigned) X(latency_path) X(lone_mid) X(by_lines)      \
  X(by_wave) X(f_sets) X(lines_buf) X(tail_wave) X(merged) X(n_pairs) X(use_msm) X(steps) X(split) X(fold)     \
  X(mtail) X(mt_wide) X(msm_wide) X(bits_lp) X(rtail) X(n_ent) X(max_chunks) X(msm_short) X(msm_T) X(lsplit)   \
  X(dec_lp) X(hf_lp) X(hash_full) X(hf_narrow) X(lines_lp) X(dec_sets) X(hf_sets) X(ll_sets) X(level_wc)       \
  X(lvl_per) X(needs_lp) X(tp_release) X(mt_out) X(fx) X(halves) X(hash) X(lines) X(decode) X(miller_wave)     \
  X(miller_sets) X(lines_W) X(step_M) X(step_W) X(acc_lpr)

extern "C" {

void pp_env_clear() { g_env.clear(); }
void pp_env_set(const char* name, const char* value) { g_env[name] = value; }

PipeConfig* pp_config_new(int from_env) {
  PipeConfig* c = new PipeConfig();
  if (from_env) config_from_env(*c, env_lookup);
  return c;
}
void pp_config_free(PipeConfig* c) { delete c; }
int pp_config_nfields() {
  int n = 0;
#define X(f) n++;
  CFG_FIELDS(X)
#undef X
  return n;
}
const char* pp_config_field(int i) {
  static const char* names[] = {
#define X(f) #f,
      CFG_FIELDS(X)
#undef X
  };
  return names[i];
}
long long pp_config_get(const PipeConfig* c, const char* name) {
#define X(f) \
  if (!strcmp(name, #f)) return (long long)c->f;
  CFG_FIELDS(X)
#undef X
  return -999;
}
int pp_env_nknobs() { return (int)(sizeof(kEnvKnobs) / sizeof(kEnvKnobs[0])); }
const char* pp_env_knob(int i) { return kEnvKnobs[i].name; }

PipePlan* pp_plan_new(const PipeConfig* c, unsigned n_req, unsigned n_sets, int lone, int partial, int presigned,
                      int prio) {
  PipeShape s;
  s.n_req = n_req;
  s.n_sets = n_sets;
  s.lone = lone;
  s.partial = partial;
  s.presigned = presigned;
  s.prio_slot = prio;
  return new PipePlan(plan_pipeline(*c, s));
}
PipePlan* pp_plan_upper_new(const PipeConfig* c, unsigned n_req, unsigned n_sets) {
  return new PipePlan(plan_upper(*c, n_req, n_sets));
}
void pp_plan_free(PipePlan* p) { delete p; }
long long pp_plan_get(const PipePlan* p, const char* name) {
#define X(f) \
  if (!strcmp(name, #f)) return (long long)p->f;
  PLAN_FIELDS(X)
#undef X
  return -999;
}

int pp_buf_count() { return PB_COUNT; }
const char* pp_buf_name(int i) { return kPipeBufNames[i]; }
// off / size: PB_COUNT entries each (absent: off = -1)
unsigned long long pp_layout(const PipePlan* p, unsigned long long start, long long* off, unsigned long long* size) {
  const PipeLayout L = layout_pipeline(*p, (size_t)start);
  for (int b = 0; b < PB_COUNT; b++) {
    off[b] = L.has((PipeBuf)b) ? (long long)L.off[b] : -1;
    size[b] = L.size[b];
  }
  return L.bytes;
}
unsigned long long pp_upper_bytes(const PipeConfig* c, unsigned n_req, unsigned n_sets) {
  return layout_pipeline(plan_upper(*c, n_req, n_sets)).bytes;
}
unsigned long long pp_lp_ws_bytes(unsigned long long ns) { return lp_ws_bytes((size_t)ns); }

}  // extern "C"

#ifdef PLAN_HOST_MAIN
static int fail(const char* what, unsigned n_req, unsigned n_sets, int cfg) {
  std::printf("FAIL %s n_req=%u n_sets=%u config=%d\n", what, n_req, n_sets, cfg);
  return 1;
}

int main() {
  const char* envs[][2][2] = {{{nullptr, nullptr}, {nullptr, nullptr}},
                              {{"LB_ACC", "pairs"}, {nullptr, nullptr}},
                              {{"LB_ACC", "pairs"}, {"LB_ACC_SPLIT", "1"}},
                              {{"LB_TAIL", "lane"}, {nullptr, nullptr}},
                              {{"LB_MTAIL", "0"}, {nullptr, nullptr}},
                              {{"LB_LEVEL", "0"}, {nullptr, nullptr}},
                              {{"LB_STEP_SPLIT", "4"}, {nullptr, nullptr}},
                              {{"LB_MSM_T_LONE", "1"}, {nullptr, nullptr}}};
  const unsigned sets[] = {0, 1, 2, 67, 68, 69, 1025, 4704, 65536, 1048576};
  int ci = 0;
  for (auto& e : envs) {
    g_env.clear();
    for (auto& kv : e)
      if (kv[0]) g_env[kv[0]] = kv[1];
    PipeConfig c;
    config_from_env(c, env_lookup);
    for (unsigned n : sets) {
      const unsigned reqs[] = {1, 8, n / 128 ? n / 128 : 1, n ? n : 1};
      for (unsigned r : reqs) {
        const size_t upper = layout_pipeline(plan_upper(c, r, n)).bytes;
        for (int m = 0; m < 8; m++) {
          PipeShape s;
          s.n_req = r;
          s.n_sets = n;
          s.lone = m & 1;
          s.partial = m & 2;
          s.presigned = m & 4;
          const PipePlan p = plan_pipeline(c, s);
          const PipeLayout L = layout_pipeline(p);
          size_t end = 0;
          for (int b = 0; b < PB_COUNT; b++) {
            if (!L.has((PipeBuf)b)) continue;
            if (L.off[b] % 256 || L.off[b] < end) return fail(kPipeBufNames[b], r, n, ci);
            end = L.off[b] + L.size[b];
          }
          if (!p.latency_path && L.bytes != end) return fail("total", r, n, ci);
          if (L.bytes > upper) return fail("upper", r, n, ci);
        }
      }
    }
    size_t prev = 0;
    for (unsigned n = 0; n <= 6000; n++) {
      const size_t u = layout_pipeline(plan_upper(c, 47, n)).bytes, v = layout_pipeline(plan_upper(c, n, 6000)).bytes;
      if (u < prev) return fail("monotone in sets", 47, n, ci);
      if (n && v < layout_pipeline(plan_upper(c, n - 1, 6000)).bytes) return fail("monotone in requests", n, 6000, ci);
      prev = u;
    }
    ci++;
  }
  std::puts("ok");
  return 0;
}
#endif
