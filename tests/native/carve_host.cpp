// lodestar_amd/csrc/bls_carve.h behind a C interface for tests/test_carve.py (g++, no HIP), and with
// -DCARVE_HOST_MAIN a stand-alone program that walks the same-message grid itself (the build
// that runs under the sanitizers).
#include <cstdio>
#include <cstring>

#include "../../lodestar_amd/csrc/bls_plan.h"

using namespace lb;

namespace {
struct Rec144 {
  char b[144];
};

// every offset of a same-message layout, in the order SM_NAMES lists them
constexpr const char* SM_NAMES[] = {
    "joff", "pk", "sigo", "sig", "msg", "seed", "areq", "asig", "rows", "in_bytes",
    "d_sig", "d_sst", "d_jpk", "d_jpkst", "d_pk96", "d_sig192", "d_jbad",
    "d_valid", "d_err", "d_mask", "d_inc", "d_agg96", "d_aggcnt", "pipe1",
    "dec_in", "dec_fl", "dec_out", "dec_ofl", "dec_pre",
    "d_rset", "d_rsig", "d_rst", "d_rmsg", "d_ridx", "d_rreq", "d_rvalid", "d_rerr", "pipe2", "ws_end",
    "h_valid", "h_err", "h_jbad", "h_jpkst", "h_rset", "h_rvalid", "h_rerr", "h_mask", "h_agg96", "h_aggcnt", "pin_end"};
constexpr int SM_N = sizeof(SM_NAMES) / sizeof(SM_NAMES[0]);
static_assert(sizeof(SmLayout) == (SM_N + SI_COUNT) * sizeof(size_t), "SM_NAMES lists every offset of SmLayout");

// the offsets in SM_NAMES' order: the inputs, then every field from in_bytes on
void sm_flat(const SmLayout& L, size_t* v) {
  memcpy(v, L.in, sizeof(L.in));
  memcpy(v + SI_COUNT, &L.in_bytes, (SM_N - SI_COUNT) * sizeof(size_t));
}

SmShape sm_shape(unsigned nj, unsigned ns, unsigned rows, int by_index, int agg, int dec, int front_only) {
  SmShape s;
  s.n_jobs = nj;
  s.n_sets = ns;
  s.sig_bytes = (size_t)ns * 96;
  s.n_rows = rows;
  s.by_index = by_index;
  s.agg = agg;
  s.dec = dec;
  s.front_only = front_only;
  const PipeConfig c;  // the pipelines' shares as bls_host.hip's pipeline_ws_bytes sizes them
  s.pipe1_bytes = layout_pipeline(plan_upper(c, nj, nj)).bytes + 255;
  s.pipe2_bytes = layout_pipeline(plan_upper(c, ns, ns)).bytes + 255;
  return s;
}
}  // namespace

extern "C" {

// A list of n declarations (kind, element size 1 / 4 / 8 / 144, count, present) laid out from
// `start` and bound to `base`: off[i] (-1: absent), addr[i] (the bound pointer - base, -1: nullptr)
// -> the layout's end; *fits: against cap
unsigned long long cv_carve(int n, const int* kind, const int* elem, const unsigned long long* count, const int* present,
                            unsigned long long start, unsigned long long cap, long long* off, long long* addr,
                            int* fits) {
  static char base[1];
  static const size_t none = kCarveAbsent;
  Carve<24> c;
  CarvePtr<const char> p[32];  // (each declared with its own element type, read back as bytes)
  for (int i = 0; i < n && i < 32; i++) {
    const CarveKind k = (CarveKind)kind[i];
    const bool pr = present[i] != 0;
    const size_t* o = &none;
    if (elem[i] == 1) o = c.add<uint8_t>(k, count[i], pr, nullptr, nullptr).off;
    if (elem[i] == 4) o = c.add<uint32_t>(k, count[i], pr, nullptr, nullptr).off;
    if (elem[i] == 8) o = c.add<const uint64_t>(k, count[i], pr, nullptr, nullptr).off;
    if (elem[i] == 144) o = c.add<Rec144>(k, count[i], pr, nullptr, nullptr).off;
    p[i] = CarvePtr<const char>{o, &c.base};
  }
  const size_t end = c.layout((size_t)start);
  *fits = c.fits((size_t)cap) ? 1 : 0;
  c.bind(base);
  for (int i = 0; i < n && i < 24; i++) {
    off[i] = c.buf[i].present ? (long long)c.buf[i].off : -1;
    const char* q = p[i];
    addr[i] = q ? (long long)(q - base) : -1;
  }
  return end;
}

int cv_sm_count() { return SM_N; }
const char* cv_sm_name(int i) { return SM_NAMES[i]; }
// out: SM_N offsets (-1: absent); p12: the two pipeline shares the layout was given
void cv_sm_layout(unsigned nj, unsigned ns, unsigned rows, int by_index, int agg, int dec, int front_only,
                  unsigned long long nr, long long* out, unsigned long long* p12) {
  const SmShape s = sm_shape(nj, ns, rows, by_index, agg, dec, front_only);
  const SmLayout L = layout_same_message(s, (size_t)nr);
  size_t v[SM_N];
  sm_flat(L, v);
  for (int i = 0; i < SM_N; i++) out[i] = v[i] == kCarveAbsent ? -1 : (long long)v[i];
  p12[0] = s.pipe1_bytes;
  p12[1] = s.pipe2_bytes;
}

// the capacity a context-owned device array takes for `need` elements when it has `cap`
unsigned cv_dev_array_cap(unsigned cap, unsigned need, unsigned floor, int doubling) {
  return dev_array_cap(cap, need, floor, doubling != 0);
}
unsigned cv_dev_array_max() { return kDevArrayMax; }

unsigned long long cv_lp_layout(unsigned long long ns, int own_status, unsigned long long start, long long* off) {
  const LpLayout L = layout_lp((size_t)ns, own_status != 0, (size_t)start);
  for (int b = 0; b < LPB_COUNT; b++) off[b] = L.off[b] == kCarveAbsent ? -1 : (long long)L.off[b];
  return L.end;
}
unsigned long long cv_lp_ws_bytes(unsigned long long ns) { return lp_ws_bytes((size_t)ns); }

// off: HB_COUNT offsets (-1: absent), then in_bytes -> end
unsigned long long cv_host_layout(unsigned nr, unsigned ns, unsigned long long n_pk, unsigned long long sig_bytes,
                                  unsigned rows, int pk_off, int by_index, long long* off) {
  HostCallShape s;
  s.n_req = nr;
  s.n_sets = ns;
  s.n_pk = n_pk;
  s.sig_bytes = sig_bytes;
  s.n_rows = rows;
  s.pk_off = pk_off;
  s.by_index = by_index;
  const HostCallLayout L = layout_host_call(s);
  for (int b = 0; b < HB_COUNT; b++) off[b] = L.off[b] == kCarveAbsent ? -1 : (long long)L.off[b];
  off[HB_COUNT] = (long long)L.in_bytes;
  return L.end;
}

}  // extern "C"

#ifdef CARVE_HOST_MAIN
static int fail(const char* what, unsigned nj, unsigned ns, int m) {
  std::printf("FAIL %s n_jobs=%u n_sets=%u flags=%d\n", what, nj, ns, m);
  return 1;
}

int main(int argc, char** argv) {
  const unsigned dec_max = argc > 1 ? (unsigned)atoi(argv[1]) : 512u;
  const unsigned jobs[] = {1, 2, 3, 257}, sets[] = {0, 1, dec_max, dec_max + 1, 5000};
  for (int m = 0; m < 8; m++) {
    size_t prev_j = 0;
    for (unsigned nj : jobs) {
      size_t prev_s = 0;
      for (unsigned ns : sets) {
        const SmShape s = sm_shape(nj, ns, (m & 1) ? 3 : 0, (m & 1) || (m & 2), m & 4, ns && ns <= dec_max, 0);
        const size_t ws_end = layout_same_message(s, ns).ws_end, pin_end = layout_same_message(s, ns).pin_end;
        for (size_t nr = 0; nr <= ns; nr += (ns > 64 ? ns / 7 : 1)) {
          const SmLayout L = layout_same_message(s, nr);
          size_t v[SM_N];
          sm_flat(L, v);
          for (size_t x : v)
            if (x != kCarveAbsent && x % 256 && x != L.pipe1 && x != L.pipe2 && x != L.ws_end && x != L.pin_end)
              return fail("alignment", nj, ns, m);
          if (L.ws_end != ws_end || L.pin_end != pin_end) return fail("totals depend on nr", nj, ns, m);
          if (L.d_rerr + nr > L.pipe2 || L.pipe2 + s.pipe2_bytes > ws_end) return fail("phase 2 past the total", nj, ns, m);
          if (L.pipe1 + s.pipe1_bytes > L.d_rset) return fail("phase 1 pipeline overlaps phase 2", nj, ns, m);
        }
        if (ws_end < prev_s) return fail("monotone in sets", nj, ns, m);
        prev_s = ws_end;
      }
      if (prev_s < prev_j) return fail("monotone in jobs", nj, 5000, m);
      prev_j = prev_s;
    }
  }
  // the primitive: a list with an absent entry and a zero count, one byte short and exact
  Carve<4> c;
  uint32_t host_in[3] = {1, 2, 3};
  Rec144 host_out[2];
  uint32_t* a = nullptr;
  auto pa = c.in(host_in, 3);
  auto pb = c.scratch<uint32_t>(5, false);
  auto pz = c.scratch<uint32_t>(0);
  auto pr = c.out(host_out, 2);
  const size_t end = c.layout(7);
  static char slab[1024];
  c.bind(slab);
  const uint32_t* ca = pa;
  uint32_t *b = pb, *z = pz;
  Rec144* r = pr;
  if (end != 512 + 288 || (const char*)ca != slab + 256 || b || (char*)z != slab + 512 || (char*)r != slab + 512 || a)
    return fail("primitive", 0, 0, 0);
  if (c.buf[0].src != host_in || c.buf[3].dst != host_out || c.buf[0].kind != CARVE_IN || c.buf[3].kind != CARVE_OUT)
    return fail("kinds", 0, 0, 0);
  if (c.fits(end - 1) || !c.fits(end)) return fail("capacity", 0, 0, 0);
  memset(r, 0, 2 * sizeof(Rec144));  // (inside the slab: the sanitizer's check of the bound pointer)
  uint8_t* extra = c.scratch<uint8_t>(1);
  if (extra || c.fits(1 << 20)) return fail("too many declarations", 0, 0, 0);
  for (size_t ns : {(size_t)1, (size_t)2, (size_t)896})
    if (lp_ws_bytes(ns) != layout_lp(ns).end || layout_lp(ns, false).end >= layout_lp(ns).end)
      return fail("lp", 0, (unsigned)ns, 0);
  // the capacity rule: never below the need, unchanged while the array fits, the table's cap
  for (const bool doubling : {true, false})
    for (const uint32_t cap : {0u, 1u, 1024u, 4096u, 4097u, 1u << 30, kDevArrayMax, 0xfffffffeu})
      for (const uint32_t need : {0u, 1u, 1023u, 1024u, 1025u, 4096u, 4097u, (1u << 30) + 1, kDevArrayMax, 0xffffffffu}) {
        const uint32_t got = dev_array_cap(cap, need, doubling ? 4096u : 1024u, doubling);
        if (got < need || (need <= cap && got != cap)) return fail("dev_array_cap", cap, need, doubling);
        if (doubling && need > cap && need <= kDevArrayMax && got > kDevArrayMax) return fail("dev_array_cap max", cap, need, 1);
      }
  std::printf("ok\n");
  return 0;
}
#endif
