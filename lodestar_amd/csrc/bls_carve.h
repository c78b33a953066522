// Carving a call's buffers out of a slab, as host arithmetic: plain C++17, no HIP
// (tests/native/carve_host.cpp).
//
// A call declares each of its buffers once -- an input copied from a host pointer, scratch, or
// an output copied to a host pointer; element type and count; whether the call has it at all --
// and lays the list out: the present buffers in the order declared, each aligned to kCarveAlign.
// The slab is sized from the end of the last one and the pointers are bound from the same
// offsets, so no size formula stands apart from the list it sizes.  An absent buffer takes no
// space and binds to nullptr.  Fixed capacity: nothing is allocated per call.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#include "bls_limits.h"

namespace lb {

// The one alignment rule of every slab (Carve, layout_pipeline, the layouts of bls_plan.h)
static constexpr size_t kCarveAlign = 256;
static constexpr size_t kCarveAbsent = ~(size_t)0;
inline constexpr size_t carve_align(size_t x) { return (x + (kCarveAlign - 1)) & ~(kCarveAlign - 1); }

// The next buffer of `bytes` behind a slab's fill `end` -> its offset (kCarveAbsent, and the
// fill as it was, for a buffer the call does not have)
inline size_t carve_take(size_t& end, size_t bytes, bool present = true) {
  if (!present) return kCarveAbsent;
  const size_t off = carve_align(end);
  end = off + bytes;
  return off;
}

// The capacity a device array owned by the context (DevArray, bls_host.hip) takes to hold `need`
// elements when it has `cap`: `cap` while that is enough.  A table (`doubling`: the pubkey and
// balance tables, which grow by appends) at least doubles, within kDevArrayMax entries; a list
// takes exactly `need`.  Either takes at least `floor`, and never less than `need`.
static constexpr uint32_t kDevArrayMax = 0x7fffffffu;
inline uint32_t dev_array_cap(uint32_t cap, uint32_t need, uint32_t floor, bool doubling) {
  if (need <= cap) return cap;
  uint64_t c = doubling ? (uint64_t)cap * 2 : need;
  if (c > kDevArrayMax) c = kDevArrayMax;
  if (c < floor) c = floor;
  return c < need ? need : (uint32_t)c;
}

enum CarveKind : uint8_t { CARVE_IN, CARVE_SCRATCH, CARVE_OUT };

struct CarveBuf {
  CarveKind kind = CARVE_SCRATCH;
  size_t bytes = 0;           // element size x count (0 when absent)
  size_t off = kCarveAbsent;  // from the slab's base, once laid out (kCarveAbsent: not present)
  const void* src = nullptr;  // CARVE_IN: the host bytes
  void* dst = nullptr;        // CARVE_OUT: where the host wants them
  bool present = false;
};

// What a declaration returns: the buffer's address once the list is laid out and bound
// (base + offset; nullptr for an absent buffer), wherever a T* is wanted
template <class T>
struct CarvePtr {
  const size_t* off;
  char* const* base;
  operator T*() const { return *off == kCarveAbsent ? nullptr : reinterpret_cast<T*>(*base + *off); }
};

template <int N>
struct Carve {
  CarveBuf buf[N + 1];  // (the last entry takes every declaration past the Nth: fits() then fails)
  int n = 0;
  size_t end = 0;  // the slab's fill after the last buffer (layout)
  char* base = nullptr;

  template <class T>
  CarvePtr<T> add(CarveKind kind, size_t count, bool present, const void* src, void* dst) {
    CarveBuf& b = buf[n < N ? n++ : (n = N + 1, N)];
    b = CarveBuf{kind, present ? sizeof(T) * count : 0, kCarveAbsent, src, dst, present};
    return CarvePtr<T>{&b.off, &base};
  }
  template <class T>
  CarvePtr<const T> in(const T* src, size_t count, bool present = true) {
    return add<const T>(CARVE_IN, count, present, src, nullptr);
  }
  template <class T>
  CarvePtr<T> scratch(size_t count, bool present = true) { return add<T>(CARVE_SCRATCH, count, present, nullptr, nullptr); }
  template <class T>
  CarvePtr<T> out(T* dst, size_t count, bool present = true) { return add<T>(CARVE_OUT, count, present, nullptr, dst); }

  // Offsets from `from` (the slab's fill when the call arrives) -> the end of the last buffer
  size_t layout(size_t from = 0) {
    end = from;
    for (int i = 0; i < n && i < N; i++) buf[i].off = carve_take(end, buf[i].bytes, buf[i].present);
    return end;
  }
  bool fits(size_t cap) const { return n <= N && end <= cap; }
  void bind(char* slab) { base = slab; }
};

// ---- layouts that more than one function binds from ----------------------------------------
// (a helper call declares its list where it runs; these are the lists that are sized in one
// place and bound in another, as named offsets)

// Record sizes of the device types (bls_host.hip pins them to sizeof with static_assert)
static constexpr size_t SZ_G2J = 288, SZ_G1J = 144, SZ_G2A = 196 /* x, y and the infinity flag */, SZ_FP12 = 576;

// The latency path's workspace (run_lp).  own_status: the call has no status buffer of the
// caller's to write the sets' statuses into.
enum LpBuf : int { LPB_PK, LPB_PK_ST, LPB_IN16, LPB_FL, LPB_SIG_ST, LPB_SETREQ, LPB_F, LPB_CNT, LPB_CLK, LPB_COUNT };
struct LpLayout {
  size_t off[LPB_COUNT];
  size_t end;
};
inline LpLayout layout_lp(size_t ns, bool own_status = true, size_t start = 0) {
  LpLayout L;
  size_t at = start;
  const size_t bytes[LPB_COUNT] = {SZ_G1J * ns, ns, 4 * ns * LB_LP_NIN * 16, 4 * ns * LB_LP_NFL, ns, 4 * ns,
                                   4 * ns * 12 * 16, 4 * (size_t)LB_LP_TREE_LEVELS * ns, 8 * 4};
  for (int b = 0; b < LPB_COUNT; b++) L.off[b] = carve_take(at, bytes[b], b != LPB_SIG_ST || own_status);
  L.end = at;
  return L;
}
// (what a slab sized by pipeline_ws_bytes must also hold, since a small call takes either path)
inline size_t lp_ws_bytes(size_t ns) { return layout_lp(ns).end; }

// A host-buffer verify call (submit_host): the package's inputs, then its three outputs.  The
// offsets hold in the slot's pinned staging and in its slab alike -- the inputs travel in one
// copy of in_bytes, the outputs come back to the same places -- and the pipeline's workspace
// begins at `end` of the slab.
struct HostCallShape {
  size_t n_req = 0, n_sets = 0;
  size_t n_pk = 0;       // keys or indices in all (pk_offsets[n_sets], or one per set)
  size_t sig_bytes = 0;  // sig_offsets[n_sets]
  size_t n_rows = 0;     // a mixed package's key rows (indices AND rows)
  bool pk_off = false, by_index = false;
};
enum HostBuf : int { HB_REQ, HB_PKO, HB_PK, HB_MSG, HB_SIGO, HB_SIG, HB_SEED, HB_ROWS, HB_VALID, HB_ERR, HB_SST, HB_COUNT };
static constexpr int HB_INPUTS = HB_VALID;  // [HB_REQ, HB_INPUTS): staged from the caller's arrays
struct HostCallLayout {
  size_t off[HB_COUNT];   // kCarveAbsent: the package has no such array
  size_t size[HB_COUNT];  // bytes
  size_t in_bytes;        // the inputs' share, a multiple of kCarveAlign
  size_t end;
};
inline HostCallLayout layout_host_call(const HostCallShape& s) {
  HostCallLayout L;
  const size_t nr1 = s.n_req ? s.n_req : 1, ns1 = s.n_sets ? s.n_sets : 1;
  size_t at = 0;
  const auto take = [&](HostBuf b, size_t bytes, bool present = true) {
    L.off[b] = carve_take(at, bytes, present);
    L.size[b] = present ? bytes : 0;
  };
  take(HB_REQ, 4 * (s.n_req + 1));
  take(HB_PKO, 4 * (s.n_sets + 1), s.pk_off);
  take(HB_PK, s.n_pk * (s.by_index ? 4 : 96));
  take(HB_MSG, s.n_sets * 32);
  take(HB_SIGO, 4 * (s.n_sets + 1));
  take(HB_SIG, s.sig_bytes);
  take(HB_SEED, 32);
  take(HB_ROWS, s.n_rows * 96, s.n_rows != 0);
  L.in_bytes = at = carve_align(at);
  take(HB_VALID, nr1);
  take(HB_ERR, nr1);
  take(HB_SST, ns1);
  L.end = at;
  return L;
}

// A host-buffer call whose sets name their keys by descriptor (lb_verify_requests_keys*): behind
// the host call's own list (from its `end`; that call is laid out with pk_off and by_index and
// no key of its own, n_pk == 0) come the key source's three arrays, staged like the inputs, and
// the indices the expansion writes, n_keys of them -- the pubkey_indices the pipeline then
// reads.  The pinned staging holds [0, in_end); the pipeline's workspace begins at `end`.
struct KeyShape {
  size_t n_sets = 0, n_pool = 0, n_bits_bytes = 0;
  size_t n_keys = 0;  // what the sets expand to in all (the host's count)
};
enum KeyBuf : int { KB_SETS, KB_POOL, KB_BITS, KB_IDX, KB_COUNT };
static constexpr int KB_INPUTS = KB_IDX;  // [KB_SETS, KB_INPUTS): staged from the caller's arrays
static constexpr size_t SZ_SET_KEYS = 20;  // sizeof(lb_set_keys)
struct KeyLayout {
  size_t off[KB_COUNT], size[KB_COUNT];
  size_t in_end;  // the staged part ends here (a multiple of kCarveAlign)
  size_t end;
};
inline KeyLayout layout_key_source(const KeyShape& s, size_t from) {
  KeyLayout L;
  size_t at = from;
  const auto take = [&](KeyBuf b, size_t bytes) {
    L.off[b] = carve_take(at, bytes);
    L.size[b] = bytes;
  };
  take(KB_SETS, s.n_sets * SZ_SET_KEYS);
  take(KB_POOL, s.n_pool * 4);
  take(KB_BITS, s.n_bits_bytes);
  L.in_end = at = carve_align(at);
  take(KB_IDX, s.n_keys * 4);
  L.end = at;
  return L;
}

// A same-message package (sm_front, sm_submit, sm_advance_launch; lb_same_message_aggregates
// runs the front alone).  The slab, in order: the inputs; what the front leaves (decoded
// signatures, the jobs' aggregated sets); phase 1's verdicts and an _agg call's buffers; the
// workspace of phase 1's pipeline (pipe1, pipe1_bytes of it); and behind that a region that
// phase 2 takes once phase 1 has retired -- the retry lists, the gathered inputs of `nr` retried
// sets, the workspace of their pipeline (pipe2, pipe2_bytes of it).  A small package's decode
// records, dead when the front's kernels are through, lie in that region too.  ws_end and
// pin_end are those of the worst case, every set retried, whatever `nr` the offsets are for.
struct SmShape {
  size_t n_jobs = 0, n_sets = 0, sig_bytes = 0, n_rows = 0;
  bool by_index = false;
  bool agg = false;         // an _agg call: mask, include flags, the jobs' signatures and counts
  bool dec = false;         // the small-package decode applies (k_lp_dec)
  bool front_only = false;  // lb_same_message_aggregates: no verdicts, no pipelines, no phase 2
  size_t pipe1_bytes = 0, pipe2_bytes = 0;  // pipeline_ws_bytes of n_jobs 1-set requests / of n_sets
};
// (SI_AREQ / SI_ASIG: the aggregated sets as requests of one set and their signature offsets,
// written by the host; SI_ROWS: a mixed package's key rows)
enum SmIn : int { SI_JOFF, SI_PK, SI_SIGO, SI_SIG, SI_MSG, SI_SEED, SI_AREQ, SI_ASIG, SI_ROWS, SI_COUNT };
struct SmLayout {
  // the inputs, in the pinned staging and in the slab alike (one copy of in_bytes)
  size_t in[SI_COUNT], in_size[SI_COUNT], in_bytes;
  // the slab
  size_t d_sig, d_sst, d_jpk, d_jpkst, d_pk96, d_sig192, d_jbad;
  size_t d_valid, d_err, d_mask, d_inc, d_agg96, d_aggcnt, pipe1;
  size_t dec_in, dec_fl, dec_out, dec_ofl, dec_pre;
  size_t d_rset, d_rsig, d_rst, d_rmsg, d_ridx, d_rreq, d_rvalid, d_rerr, pipe2;
  size_t ws_end;
  // the pinned staging behind the inputs: phase 1's four result rows, the retry lists (set
  // indices, then job indices) and outputs, an _agg call's mask and outputs
  size_t h_valid, h_err, h_jbad, h_jpkst, h_rset, h_rvalid, h_rerr, h_mask, h_agg96, h_aggcnt;
  size_t pin_end;
};
inline SmLayout layout_same_message(const SmShape& s, size_t nr) {
  SmLayout L;
  const size_t nj = s.n_jobs, ns = s.n_sets, ns1 = ns ? ns : 1;
  const bool full = !s.front_only;
  size_t at = 0;
  const auto input = [&](SmIn b, size_t bytes, bool present = true) {
    L.in[b] = carve_take(at, bytes, present);
    L.in_size[b] = present ? bytes : 0;
  };
  input(SI_JOFF, 4 * (nj + 1));
  input(SI_PK, ns * (s.by_index ? 4 : 96));
  input(SI_SIGO, 4 * (ns + 1));
  input(SI_SIG, s.sig_bytes);
  input(SI_MSG, nj * 32);
  input(SI_SEED, 32);
  input(SI_AREQ, 4 * (nj + 1));
  input(SI_ASIG, 4 * (nj + 1));
  input(SI_ROWS, s.n_rows * 96, s.n_rows != 0);
  L.in_bytes = at = carve_align(at);
  size_t pin = at;
  L.d_sig = carve_take(at, ns1 * SZ_G2J);
  L.d_sst = carve_take(at, ns1);
  L.d_jpk = carve_take(at, nj * SZ_G1J);
  L.d_jpkst = carve_take(at, nj);
  L.d_pk96 = carve_take(at, nj * 96);
  L.d_sig192 = carve_take(at, nj * 192);
  L.d_jbad = carve_take(at, nj);
  L.d_valid = carve_take(at, nj, full);
  L.d_err = carve_take(at, nj, full);
  L.d_mask = carve_take(at, ns1, s.agg);
  L.d_inc = carve_take(at, ns1, s.agg);
  L.d_agg96 = carve_take(at, nj * 96, s.agg);
  L.d_aggcnt = carve_take(at, nj * 4, s.agg);
  L.pipe1 = at;
  const size_t late = at + (full ? s.pipe1_bytes : 0);
  at = late;
  L.dec_in = carve_take(at, ns * 4 * 16 * 4, s.dec);
  L.dec_fl = carve_take(at, ns * 3 * 4, s.dec);
  L.dec_out = carve_take(at, ns * 2 * 16 * 4, s.dec);
  L.dec_ofl = carve_take(at, ns * 2 * 4, s.dec);
  L.dec_pre = carve_take(at, ns, s.dec);
  L.ws_end = at;
  for (const size_t r : {ns, nr}) {  // the worst case for the total, then the call's own offsets
    at = late;
    L.d_rset = carve_take(at, 2 * ns * 4, full);
    L.d_rsig = carve_take(at, r * SZ_G2J, full);
    L.d_rst = carve_take(at, r, full);
    L.d_rmsg = carve_take(at, r * 32, full);
    L.d_ridx = carve_take(at, r * 4, full);
    L.d_rreq = carve_take(at, (r + 1) * 4, full);
    L.d_rvalid = carve_take(at, r, full);
    L.d_rerr = carve_take(at, r, full);
    L.pipe2 = at;
    if (full && at + s.pipe2_bytes > L.ws_end) L.ws_end = at + s.pipe2_bytes;
  }
  L.h_valid = carve_take(pin, nj);
  L.h_err = carve_take(pin, nj);
  L.h_jbad = carve_take(pin, nj);
  L.h_jpkst = carve_take(pin, nj);
  L.h_rset = carve_take(pin, 2 * ns1 * 4, full);
  L.h_rvalid = carve_take(pin, ns1, full);
  L.h_rerr = carve_take(pin, ns1, full);
  L.h_mask = carve_take(pin, ns1, s.agg);
  L.h_agg96 = carve_take(pin, nj * 96, s.agg);
  L.h_aggcnt = carve_take(pin, nj * 4, s.agg);
  L.pin_end = pin;
  return L;
}

}  // namespace lb
