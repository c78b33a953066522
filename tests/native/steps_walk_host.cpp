// Host build of lodestar_amd/csrc/bls_steps_walk.h (the lane walk of the step-major accumulation)
// and of the plan's pair_pre rule (bls_plan.h) for tests/test_steps_walk.py (ctypes), and with
// -DSTEPS_WALK_HOST_MAIN a stand-alone program that walks every lane of every request size itself
// (the build that runs under -fsanitize=address,undefined).
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../lodestar_amd/csrc/bls_plan.h"
#include "../../lodestar_amd/csrc/bls_steps_walk.h"

using namespace lb;

static std::map<std::string, std::string> g_env;
static const char* env_lookup(const char* name) {
  auto it = g_env.find(name);
  return it == g_env.end() ? nullptr : it->second.c_str();
}

extern "C" {

// The lane's items -> out[3 k ..] = (j, i, paired); returns their count (at most L)
int sw_items(unsigned n, unsigned t0, unsigned L, int pairs, unsigned* out) {
  StepWalk w(n, t0, L, pairs != 0);
  int k = 0;
  while (!w.done()) {
    const StepItem it = w.next();
    out[3 * k] = it.j;
    out[3 * k + 1] = it.i;
    out[3 * k + 2] = it.paired;
    k++;
  }
  return k;
}
int sw_pair_at(unsigned n, unsigned t0, unsigned L, unsigned u, unsigned* ji) {
  uint32_t j = 0xffffffffu, i = 0xffffffffu;
  const bool ok = step_walk_pair(n, t0, L, u, j, i);
  ji[0] = j;
  ji[1] = i;
  return ok;
}

void sw_env_clear() { g_env.clear(); }
void sw_env_set(const char* name, const char* value) { g_env[name] = value; }
// plan_pipeline's pair_pre of a call under the table's environment; what = 1: its step_M, 2: lines, 3: steps
int sw_plan(unsigned n_req, unsigned n_sets, int lone, int partial, int what) {
  PipeConfig c;
  config_from_env(c, env_lookup);
  PipeShape s;
  s.n_req = n_req;
  s.n_sets = n_sets;
  s.lone = lone;
  s.partial = partial;
  const PipePlan p = plan_pipeline(c, s);
  return what == 1 ? p.step_M : what == 2 ? (int)p.lines : what == 3 ? (int)p.steps : (int)p.pair_pre;
}
int sw_pair_pre_compiled() { return LB_PAIR_PRE; }
unsigned sw_pair_pre_min_sets() { return LB_PAIR_PRE_MIN_SETS; }
int sw_lines_rows() { return LINES_ROWS; }

}  // extern "C"

#ifdef STEPS_WALK_HOST_MAIN
static int fail(const char* what, unsigned n, unsigned L, unsigned lane) {
  std::printf("FAIL %s n=%u L=%u lane=%u\n", what, n, L, lane);
  return 1;
}

int main() {
  const unsigned Ls[] = {68, 34, 17};
  for (unsigned n = 1; n <= 130; n++)
    for (unsigned L : Ls) {
      std::vector<int> seen(68 * n, 0);
      for (unsigned lane = 0; lane < 68 * n / L; lane++) {
        std::vector<unsigned> out(3 * L);
        const int k = sw_items(n, lane * L, L, 1, out.data());
        unsigned pairs = 0, lines = 0;
        for (int e = 0; e < k; e++) {
          const unsigned j = out[3 * e], i = out[3 * e + 1], two = out[3 * e + 2];
          if (j >= 68 || i + two >= n) return fail("range", n, L, lane);
          if (j * n + i != lane * L + lines) return fail("order", n, L, lane);
          for (unsigned d = 0; d <= two; d++) seen[j * n + i + d]++;
          lines += 1 + two;
          if (two) {
            unsigned ji[2];
            if (!sw_pair_at(n, lane * L, L, pairs, ji) || ji[0] != j || ji[1] != i) return fail("pair_at", n, L, lane);
            pairs++;
          }
        }
        unsigned ji[2];
        if (lines != L || pairs > L / 2 || sw_pair_at(n, lane * L, L, pairs, ji)) return fail("count", n, L, lane);
        if (sw_items(n, lane * L, L, 0, out.data()) != (int)L) return fail("singles", n, L, lane);
      }
      for (int s : seen)
        if (s != 1) return fail("cover", n, L, 0);
    }
  for (unsigned sets : {8191u, 8192u})
    for (int lone = 0; lone < 2; lone++)
      for (const char* mode : {"0", "1", "2"}) {
        sw_env_clear();
        sw_env_set("LB_STEP_MODE", mode);
        const int want = LB_PAIR_PRE && sets >= LB_PAIR_PRE_MIN_SETS && mode[0] != '2';
        if (sw_plan(64, sets, lone, 0, 0) != want) return fail("pair_pre", sets, (unsigned)lone, (unsigned)(mode[0] - '0'));
      }
  std::puts("ok");
  return 0;
}
#endif
