// N-API addon: the Lodestar-side binding of the MI355X BLS verifier C ABI
// (include/lodestar_bls.h).  This is what a BlsGpuVerifier beside
// BlsMultiThreadWorkerPool (packages/beacon-node/src/chain/bls, chosen at
// BN/chain/chain.ts:206-208) requires: it replaces the worker boundary
// workerApi.verifyManySignatureSets(workReqs) (chain/bls/multithread/index.ts:444,
// worker.ts:24-30) with one call per package on a GPU.
//
// Threading: JS calls arrive on the main thread; their
// offsets are copied there (the reference structured-clones its requests to the
// worker, index.ts:444), the bulk arrays of verifyRequests are read in place (kept
// alive by references until the promise settles: the caller must not modify them
// meanwhile), and the task goes to ONE host submission thread per GPU, which owns
// the lb_ctx (not thread-safe) and keeps up to `capacity` calls in flight
// (lb_verify_requests_async + lb_wait).  Completions come back to the event
// loop through a threadsafe function; the event loop never blocks on the GPU.
// Every native method returns a Promise; bad arguments and device errors
// reject it (a malformed signature is a verdict, never an error).
//
// Every operation is one struct derived from Task (below): its inputs and outputs under
// their own names, run() for the submission thread, mirror() where the latency lane's
// context has to follow, result() for the event loop -- and one entry point that parses
// its arguments (method<T>).  The scheduling knows no operation by name; it runs under
// node without a GPU against tests/native/lb_stub.c (tests/js/addon_sched.js).
//
// Exports (lodestar_amd/js/index.d.ts has the types):
//   deviceCount() -> number
//   validateRequests(batch) -> {nRequests, nSets, nPubkeys, byIndex}   (marshalling dry run, no device)
//   new Context(device, {capacity?, sameMessageRandomized?})
//                                    (throws Error{code: "LB_ERR_NO_DEVICE", ...} without a GPU)
//     .verifyRequests(batch, {priority?}) -> Promise<{valid, errors, setStatus, batchRetries,
//                                        batchSigsSuccess, deviceMs, workerStartNs, workerEndNs,
//                                        workerSubmittedNs, workerRetireNs}>
//         (priority: the device's priority lane -- started at once, beside the calls in
//          flight, retired as soon as it completes; lb_verify_requests_priority_async.  On the
//          latency lane the result also has kernelMs and kernelClockMHz, and stageMs: {stage: ms}
//          with LB_STAGE_EVENTS=1)
//     .verifyRequestsPartial(batch) -> Promise<{id, partial: Uint8Array(576)}>  (two-phase, multi-GPU)
//     .finish(id, mergedOk) -> Promise<result of verifyRequests>
//     .gtCheck(Uint8Array n*576) -> Promise<boolean>
//     .verifySameMessage({jobOffsets, pubkeys|pubkeyIndices, signatures, sigOffsets, messages, seed})
//         -> Promise<{valid, jobFast, retriedJobs, fastSets, deviceMs, workerStartNs, workerEndNs}>
//     .verifySameMessage(batch, {aggregate: true, mask?: Uint8Array(nSets)})
//         -> the same plus {jobSignatures: Uint8Array(nJobs*96), jobCounts: Uint32Array(nJobs)}: each
//            job's valid (and mask-kept) signatures summed, compressed (lb_verify_same_message_batch_agg_async)
//     .aggregateSignatureGroups({groupOffsets, signatures, sigOffsets}, {noCheck?})
//         -> Promise<{signatures: Uint8Array(nGroups*96), badIndex: Int32Array(nGroups)}>
//     .kzgLoadSetup(Uint8Array(96)) -> Promise<void>                  (KZG_SETUP_G2_MONOMIAL[1], compressed)
//     .kzgVerifyBlobProofBatch(blobs n*131072, commitments n*48, proofs n*48: Uint8Array)
//         -> Promise<{ok: boolean, status: Uint8Array(n)}>             (verifyBlobKzgProofBatch; status LB_KZG_*)
//     .kzgLoadSetupG1(Uint8Array(196608)) -> Promise<void>            (the 4096 G1 Lagrange lines, file order)
//     .kzgBlobCommitments(blobs) -> Promise<{commitments: Uint8Array(n*48), status}>   (blobToKzgCommitment)
//     .kzgBlobProofs(blobs, commitments) -> Promise<{proofs: Uint8Array(n*48), status}> (computeBlobKzgProof)
//     .kzgComputeProofs(blobs, zs n*32) -> Promise<{proofs, ys: Uint8Array(n*32), status}> (computeKzgProof)
//     .syncPubkeys(Uint8Array keys, pkLen) -> Promise<number>          (index2pubkey mirror; the table's size)
//     .aggregatePubkeys(Uint8Array n*96 | Uint32Array indices) -> Promise<Uint8Array(96)>
//     .indexListPut(listId, indices: Uint32Array) -> Promise<number>   (the list's length)
//     .indexListShuffle(listId, activeIndices: Uint32Array, seed: Uint8Array(32)) -> Promise<Uint32Array>
//         (the shuffling, which list `listId` now holds)
//     .balanceTablePut(first, increments: Uint8Array) -> Promise<number>   (the table's size)
//     .sampleByBalance({seeds: Uint8Array(32 k), count, activeIndices: Uint32Array, maxIncrement,
//                       maxCandidates, storeList?, aggregate?})
//         -> Promise<{indices: Uint32Array(k*count), found, tried: Uint32Array(k), aggregatePubkey?}>
//     .close() -> Promise<void>                                      (waits for calls in flight)
//   batch = {requestOffsets: Uint32Array, pubkeys?: Uint8Array, pubkeyIndices?: Uint32Array,
//            pkOffsets?: Uint32Array, messages: Uint8Array, signatures: Uint8Array,
//            sigOffsets: Uint32Array, seed: Uint8Array(32), batchable?: Uint8Array}
//        or, the sets' keys by descriptor (lb_key_source) instead of pubkeys / pkOffsets / pubkeyIndices:
//           {..., setKeys: Uint32Array(5 per set: kind, list, a, len, bitsOff), keyPool?: Uint32Array,
//            keyBits?: Uint8Array}
#define NAPI_VERSION 8
#include <node_api.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/lodestar_bls.h"

namespace {

#define NAPI_OK(call)                       \
  do {                                      \
    if ((call) != napi_ok) return nullptr;  \
  } while (0)

struct ArgError {
  std::string msg;
};

uint64_t now_ns() {
  return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// ---- marshalling: JS -> C ----------------------------------------------------------
bool has_prop(napi_env env, napi_value obj, const char* name, napi_value* out) {
  bool has = false;
  if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return false;
  if (napi_get_named_property(env, obj, name, out) != napi_ok) return false;
  napi_valuetype t;
  napi_typeof(env, *out, &t);
  return t != napi_undefined && t != napi_null;
}

bool is_object(napi_env env, napi_value v) {
  napi_valuetype t = napi_undefined;
  napi_typeof(env, v, &t);
  return t == napi_object;
}

// options.name as a boolean, when argv[i] is an object that has it
void opt_bool(napi_env env, size_t argc, napi_value* argv, size_t i, const char* name, bool* out) {
  napi_value v;
  if (argc > i && is_object(env, argv[i]) && has_prop(env, argv[i], name, &v)) napi_get_value_bool(env, v, out);
}

struct ArrayInfo {
  napi_typedarray_type type;
  void* data;
  size_t len;  // elements
};
ArrayInfo array_info(napi_env env, napi_value v, const char* name) {
  bool is = false;
  napi_is_typedarray(env, v, &is);
  if (!is) throw ArgError{std::string(name) + " must be a typed array"};
  ArrayInfo a{};
  napi_value ab;
  size_t off = 0;
  napi_get_typedarray_info(env, v, &a.type, &a.len, &a.data, &ab, &off);
  return a;
}
// a Uint8Array (clamped or not) or a Uint32Array, as `want` says
ArrayInfo array_of(napi_env env, napi_value v, napi_typedarray_type want, const char* name) {
  const ArrayInfo a = array_info(env, v, name);
  if (a.type != want && !(want == napi_uint8_array && a.type == napi_uint8_clamped_array))
    throw ArgError{std::string(name) + (want == napi_uint8_array ? " must be a Uint8Array" : " must be a Uint32Array")};
  return a;
}

template <class T>
void typed(napi_env env, napi_value v, napi_typedarray_type want, const char* name, std::vector<T>& out) {
  const ArrayInfo a = array_of(env, v, want, name);
  out.resize(a.len);
  if (a.len) memcpy(out.data(), a.data, a.len * sizeof(T));
}

template <class T>
void req_typed(napi_env env, napi_value obj, const char* name, napi_typedarray_type want, std::vector<T>& out) {
  napi_value v;
  if (!has_prop(env, obj, name, &v)) throw ArgError{std::string("missing ") + name};
  typed(env, v, want, name, out);
}

template <class T>
bool opt_typed(napi_env env, napi_value obj, const char* name, napi_typedarray_type want, std::vector<T>& out) {
  napi_value v;
  if (!has_prop(env, obj, name, &v)) return false;
  typed(env, v, want, name, out);
  return true;
}

// A typed array read in place (no copy on the JS thread): the caller's buffer, kept
// alive by a reference the JS thread releases when the task settles.  Used for the
// bulk inputs of verifyRequests (messages, signatures, pubkeys, pubkeyIndices: ~8 MB
// for a 65,536-set package, ~1 ms of main-thread memcpy); the caller must not modify
// them until the promise settles (packRequests' arrays are fresh and private).
template <class T>
struct View {
  const T* p = nullptr;
  size_t n = 0;
  std::vector<T> own;  // a copy instead (empty-array placeholder)
  const T* data() const { return p ? p : own.data(); }
  size_t size() const { return p ? n : own.size(); }
  bool empty() const { return size() == 0; }
};

template <class T>
void typed_view(napi_env env, napi_value v, napi_typedarray_type want, const char* name, View<T>& out,
                std::vector<napi_ref>& refs) {
  const ArrayInfo a = array_of(env, v, want, name);
  napi_ref r = nullptr;
  if (a.len && napi_create_reference(env, v, 1, &r) == napi_ok) {
    refs.push_back(r);
    out.p = static_cast<const T*>(a.data);
    out.n = a.len;
  } else {
    out.p = nullptr;
    out.own.assign(static_cast<const T*>(a.data), static_cast<const T*>(a.data) + a.len);
  }
}

// Every pointer handed to the library is valid: an empty input gets one placeholder
// element, an output of no elements is allocated as one (the counts stay 0).
template <class T>
void pad(std::vector<T>& v) {
  if (v.empty()) v.push_back(0);
}
template <class T>
void pad(View<T>& v) {
  if (v.empty()) v.own.assign(1, 0);
}
template <class T>
void alloc_out(std::vector<T>& v, size_t n, T fill = 0) {
  v.assign(n ? n : 1, fill);
}

void check_offsets(const std::vector<uint32_t>& off, size_t n, uint32_t last, const char* name) {
  if (off.size() != n + 1) throw ArgError{std::string(name) + ": wrong length"};
  if (off[0] != 0) throw ArgError{std::string(name) + " must start at 0"};
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) throw ArgError{std::string(name) + " not monotone"};
  if (last != UINT32_MAX && off[n] != last) throw ArgError{std::string(name) + ": wrong end"};
}

// a batch's or a shuffling's seed: 32 bytes
void seed32(napi_env env, napi_value v, std::vector<uint8_t>& out) {
  typed(env, v, napi_uint8_array, "seed", out);
  if (out.size() != 32) throw ArgError{"seed must be 32 bytes"};
}

// Mixed package: the rows of `pubkeys` that indices with LB_PK_ROW_FLAG name
size_t pk_rows_needed(const uint32_t* ix, size_t n) {
  size_t rows = 0;
  for (size_t q = 0; q < n; q++)
    if ((ix[q] & LB_PK_ROW_FLAG) && (size_t)(ix[q] & LB_PK_ROW_MASK) + 1 > rows) rows = (ix[q] & LB_PK_ROW_MASK) + 1;
  return rows;
}
void check_pk_rows(const uint32_t* ix, size_t n, bool has_keys, size_t key_bytes) {
  const size_t rows = pk_rows_needed(ix, n);
  if (rows && (!has_keys || key_bytes < rows * LB_PUBKEY_BYTES))
    throw ArgError{"pubkeyIndices name pubkey rows that `pubkeys` does not hold"};
}

// blobs: n x 131072 bytes; returns n
uint32_t parse_blobs(napi_env env, napi_value v, std::vector<uint8_t>& blobs) {
  typed(env, v, napi_uint8_array, "blobs", blobs);
  if (blobs.size() % LB_KZG_BLOB_BYTES) throw ArgError{"blobs: 131072 bytes each"};
  const size_t n = blobs.size() / LB_KZG_BLOB_BYTES;
  if (n > LB_KZG_MAX_BLOBS) throw ArgError{"blobs: more than LB_KZG_MAX_BLOBS"};
  pad(blobs);
  return (uint32_t)n;
}
// a second array of `each` bytes per blob
void parse_per_blob(napi_env env, napi_value v, const char* name, size_t each, uint32_t n, const char* rule,
                    std::vector<uint8_t>& out) {
  typed(env, v, napi_uint8_array, name, out);
  if (out.size() != (size_t)n * each) throw ArgError{rule};
  pad(out);
}

// ---- marshalling: C -> JS ----------------------------------------------------------
napi_value make_u8(napi_env env, const uint8_t* p, size_t n) {
  napi_value ab, arr;
  void* data = nullptr;
  NAPI_OK(napi_create_arraybuffer(env, n, &data, &ab));
  if (n) memcpy(data, p, n);
  NAPI_OK(napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &arr));
  return arr;
}

// n 32-bit words as a Uint32Array / Int32Array
napi_value make_words(napi_env env, napi_typedarray_type ty, const void* p, size_t n) {
  void* data = nullptr;
  napi_value ab, arr;
  napi_create_arraybuffer(env, n * 4, &data, &ab);
  if (n) memcpy(data, p, n * 4);
  napi_create_typedarray(env, ty, n, ab, 0, &arr);
  return arr;
}
napi_value make_u32s(napi_env env, const std::vector<uint32_t>& v, size_t n) {
  return make_words(env, napi_uint32_array, v.data(), n);
}

napi_value make_object(napi_env env) {
  napi_value o;
  napi_create_object(env, &o);
  return o;
}
napi_value make_uint(napi_env env, uint32_t v) {
  napi_value x;
  napi_create_uint32(env, v, &x);
  return x;
}
napi_value make_bool(napi_env env, bool v) {
  napi_value x;
  napi_get_boolean(env, v, &x);
  return x;
}
napi_value make_undefined(napi_env env) {
  napi_value x;
  napi_get_undefined(env, &x);
  return x;
}
void set(napi_env env, napi_value obj, const char* k, napi_value v) { napi_set_named_property(env, obj, k, v); }
void set_num(napi_env env, napi_value obj, const char* k, double v) {
  napi_value x;
  napi_create_double(env, v, &x);
  napi_set_named_property(env, obj, k, x);
}

napi_value make_error(napi_env env, int rc, const std::string& msg) {
  const char* code = rc == LB_ERR_INVALID_ARGUMENT ? "LB_ERR_INVALID_ARGUMENT"
                     : rc == LB_ERR_DEVICE         ? "LB_ERR_DEVICE"
                     : rc == LB_ERR_NO_DEVICE      ? "LB_ERR_NO_DEVICE"
                     : rc == LB_ERR_OUT_OF_MEMORY  ? "LB_ERR_OUT_OF_MEMORY"
                     : rc == LB_ERR_RESOURCES      ? "LB_ERR_RESOURCES"
                                                   : "LB_ERR";
  napi_value c, m, e;
  napi_create_string_utf8(env, code, NAPI_AUTO_LENGTH, &c);
  napi_create_string_utf8(env, msg.c_str(), NAPI_AUTO_LENGTH, &m);
  napi_create_error(env, c, m, &e);
  return e;
}

// ---- tasks ---------------------------------------------------------------------------
// What an asynchronous library call is retired by: its ticket, and where lb_wait puts its stats.
struct Ticket {
  uint64_t id = 0;
  lb_verify_stats stats{0, 0, 0.0};
};

// One JS call on its way through the threads: created and parsed on the JS thread
// (method<T>), run on the submission thread, for some operations repeated on the lane
// thread, settled on the JS thread (call_js).  A derived struct adds the operation's own
// inputs and outputs.  What holds for every task:
//   - napi_refs are created and deleted on the JS thread only (refs travel with the task;
//     release_refs runs in method<T>, submit, call_js and finalize_ctx);
//   - a task is deleted on the JS thread (call_js), or in the finalize paths (complete /
//     lane_loop / finalize_ctx once Context::finalizing is set);
//   - the input views (kept alive by refs) and the output vectors of a call in flight live
//     until lb_wait for its ticket has returned: the library reads and writes them until then;
//   - run() is called by the submission thread alone, with Context::ctx; mirror() by the lane
//     thread alone, with Context::lctx.  Neither context is touched by any other thread
//     (lb_mark_priority excepted, which the library allows).
struct Task {
  napi_deferred deferred = nullptr;
  std::vector<napi_ref> refs;  // the input arrays read in place (View)
  bool prio = false;           // verifyRequests(batch, {priority: true}): the device's priority lane
  bool close = false;          // close(): startable at any time, and the last task of its context
  int rc = LB_OK;
  std::string errmsg;    // with rc: what the promise rejects with
  std::string err_note;  // appended to the library's message by fail() (which input it refused)
  // steady-clock ns: run() about to be called; for a one-phase verify call, its submit returned and
  // lb_wait about to be called; the task about to be completed
  uint64_t t_start = 0, t_submitted = 0, t_retire = 0, t_end = 0;

  virtual ~Task() {}
  // The operation, on the context it is given.  LB_OK, or an error the caller records with
  // fail(); an error that is the task's own (no library message) is put into rc / errmsg.
  virtual int run(lb_ctx* ctx) = 0;
  // Non-null once run() has put a library call in flight (verify, finish, same-message): the
  // task is then retired by lb_wait on it, in submission order, instead of completing at once.
  virtual Ticket* ticket() { return nullptr; }
  // What of the lane's context has to follow this task after a successful run() (nullptr:
  // nothing), and the call that makes it follow.
  virtual const char* mirror_what() const { return nullptr; }
  virtual int mirror(lb_ctx* /*lane*/) { return LB_OK; }
  // The value the promise resolves with (JS thread, rc == LB_OK).
  virtual napi_value result(napi_env env) = 0;
};

void release_refs(napi_env env, std::vector<napi_ref>& refs) {
  for (napi_ref r : refs) napi_delete_reference(env, r);
  refs.clear();
}

void fail(Task* t, int rc, lb_ctx* ctx) {
  t->rc = rc;
  t->errmsg = (ctx ? lb_last_error(ctx) : "no context") + t->err_note;
}
int own_error(Task* t, const char* msg) {
  t->rc = LB_ERR_INVALID_ARGUMENT;
  t->errmsg = msg;
  return LB_OK;
}

// ---- verifyRequests / verifyRequestsPartial / finish -----------------------------------------
// A parsed batch: offsets copied, bulk arrays read in place.
struct Requests {
  uint32_t n_req = 0, n_sets = 0;
  std::vector<uint32_t> req_off, pk_off, sig_off;
  std::vector<uint8_t> seed, batchable;
  View<uint8_t> pubkeys, messages, signatures;
  View<uint32_t> pk_idx;
  bool has_pk_off = false, by_index = false, has_batchable = false, mixed = false;
  // {setKeys, keyPool, keyBits, ...}: the sets' keys by descriptor (lb_key_source);
  // set_keys holds five words per set (lb_set_keys: kind, list, a, len, bits_off)
  bool by_keys = false;
  std::vector<uint32_t> set_keys, key_pool;
  std::vector<uint8_t> key_bits;

  size_t n_pubkeys() const { return has_pk_off ? pk_off[n_sets] : n_sets; }
  lb_request_batch batch() const {
    lb_request_batch b{};
    b.n_requests = n_req;
    b.n_sets = n_sets;
    b.request_offsets = req_off.data();
    b.request_batchable = has_batchable ? batchable.data() : nullptr;
    b.pubkeys = by_keys ? nullptr : (!by_index || mixed) ? pubkeys.data() : nullptr;
    b.pk_offsets = has_pk_off ? pk_off.data() : nullptr;
    b.messages = messages.data();
    b.signatures = signatures.data();
    b.sig_offsets = sig_off.data();
    b.seed = seed.data();
    b.pubkey_indices = by_index ? pk_idx.data() : nullptr;
    return b;
  }
  lb_key_source keys() const {
    static const uint32_t none32 = 0;
    static const uint8_t none8 = 0;
    lb_key_source k{};
    k.sets = reinterpret_cast<const lb_set_keys*>(set_keys.empty() ? &none32 : set_keys.data());
    k.key_pool = key_pool.empty() ? &none32 : key_pool.data();
    k.n_pool = (uint32_t)key_pool.size();
    k.bits = key_bits.empty() ? &none8 : key_bits.data();
    k.n_bits_bytes = (uint32_t)key_bits.size();
    return k;
  }
};
static_assert(sizeof(lb_set_keys) == 5 * sizeof(uint32_t), "setKeys rows are lb_set_keys");

void parse_requests(napi_env env, napi_value obj, Requests& t, std::vector<napi_ref>& refs) {
  if (!is_object(env, obj)) throw ArgError{"batch must be an object"};
  req_typed(env, obj, "requestOffsets", napi_uint32_array, t.req_off);
  if (t.req_off.empty()) throw ArgError{"requestOffsets: wrong length"};
  t.n_req = (uint32_t)t.req_off.size() - 1;
  t.n_sets = t.req_off.back();
  check_offsets(t.req_off, t.n_req, UINT32_MAX, "requestOffsets");
  napi_value mv, sv, seedv;
  if (!has_prop(env, obj, "messages", &mv)) throw ArgError{"missing messages"};
  typed_view(env, mv, napi_uint8_array, "messages", t.messages, refs);
  if (t.messages.size() != (size_t)t.n_sets * 32) throw ArgError{"messages: 32 bytes per set"};
  if (!has_prop(env, obj, "signatures", &sv)) throw ArgError{"missing signatures"};
  typed_view(env, sv, napi_uint8_array, "signatures", t.signatures, refs);
  req_typed(env, obj, "sigOffsets", napi_uint32_array, t.sig_off);
  check_offsets(t.sig_off, t.n_sets, (uint32_t)t.signatures.size(), "sigOffsets");
  if (!has_prop(env, obj, "seed", &seedv)) throw ArgError{"missing seed"};
  seed32(env, seedv, t.seed);
  t.by_keys = opt_typed(env, obj, "setKeys", napi_uint32_array, t.set_keys);
  if (t.by_keys) {
    // keys by descriptor: nothing else names a key (the library checks every bound at submit)
    napi_value x;
    if (has_prop(env, obj, "pkOffsets", &x) || has_prop(env, obj, "pubkeyIndices", &x) || has_prop(env, obj, "pubkeys", &x))
      throw ArgError{"setKeys excludes pubkeys, pkOffsets and pubkeyIndices"};
    if (t.set_keys.size() != (size_t)t.n_sets * 5) throw ArgError{"setKeys: five words per set"};
    opt_typed(env, obj, "keyPool", napi_uint32_array, t.key_pool);
    opt_typed(env, obj, "keyBits", napi_uint8_array, t.key_bits);
  } else {
    t.has_pk_off = opt_typed(env, obj, "pkOffsets", napi_uint32_array, t.pk_off);
    if (t.has_pk_off) check_offsets(t.pk_off, t.n_sets, UINT32_MAX, "pkOffsets");
    const size_t n_pk = t.n_pubkeys();
    napi_value iv, kv;
    t.by_index = has_prop(env, obj, "pubkeyIndices", &iv);
    const bool has_keys = has_prop(env, obj, "pubkeys", &kv);
    if (has_keys) typed_view(env, kv, napi_uint8_array, "pubkeys", t.pubkeys, refs);
    if (t.by_index) {
      typed_view(env, iv, napi_uint32_array, "pubkeyIndices", t.pk_idx, refs);
      if (t.pk_idx.size() != n_pk) throw ArgError{"pubkeyIndices: one index per pubkey"};
      t.mixed = has_keys;
      check_pk_rows(t.pk_idx.data(), n_pk, t.mixed, t.pubkeys.size());
    } else {
      if (!has_keys && n_pk) throw ArgError{"missing pubkeys (or pubkeyIndices)"};
      if (t.pubkeys.size() != n_pk * LB_PUBKEY_BYTES) throw ArgError{"pubkeys: 96 bytes per pubkey"};
    }
    pad(t.pubkeys);
    pad(t.pk_idx);
  }
  t.has_batchable = opt_typed(env, obj, "batchable", napi_uint8_array, t.batchable);
  if (t.has_batchable && t.batchable.size() != t.n_req) throw ArgError{"batchable: one flag per request"};
  pad(t.signatures);
  pad(t.messages);
}

// One verify call of the library: its batch, its outputs, its ticket.  A one-phase call is part
// of its task; a two-phase call lives in Context::partials between the promise that
// verifyRequestsPartial resolves and the finish() that retires it.
struct VerifyCall {
  Requests in;
  std::vector<uint8_t> valid, err, sst;
  Ticket tk;
  // two-phase: the partial's start, and its inputs' references while no task holds them
  uint64_t t_start = 0;
  std::vector<napi_ref> refs;

  enum Mode { ASYNC, PRIORITY, PARTIAL };
  // in the form the batch came in (keys by descriptor: the _keys_ entry points)
  int submit(lb_ctx* ctx, Mode mode) {
    alloc_out(valid, in.n_req);
    alloc_out(err, in.n_req);
    alloc_out(sst, in.n_sets);
    const lb_request_batch b = in.batch();
    uint8_t *v = valid.data(), *e = err.data(), *s = sst.data();
    if (in.by_keys) {
      const lb_key_source k = in.keys();
      return mode == PRIORITY  ? lb_verify_requests_keys_priority_async(ctx, &b, &k, v, e, s, &tk.id)
             : mode == PARTIAL ? lb_verify_requests_keys_partial_async(ctx, &b, &k, v, e, s, &tk.id)
                               : lb_verify_requests_keys_async(ctx, &b, &k, v, e, s, &tk.id);
    }
    return mode == PRIORITY  ? lb_verify_requests_priority_async(ctx, &b, v, e, s, &tk.id)
           : mode == PARTIAL ? lb_verify_requests_partial_async(ctx, &b, 0, v, e, s, &tk.id)
                             : lb_verify_requests_async(ctx, &b, v, e, s, &tk.id);
  }
  // the verdicts of a retired call, with the stamps of the task that resolves with them
  napi_value verdicts(napi_env env, const Task& t, bool one_phase) const {
    napi_value o = make_object(env);
    set(env, o, "valid", make_u8(env, valid.data(), in.n_req));
    set(env, o, "errors", make_u8(env, err.data(), in.n_req));
    set(env, o, "setStatus", make_u8(env, sst.data(), in.n_sets));
    set_num(env, o, "batchRetries", tk.stats.batch_retries);
    set_num(env, o, "batchSigsSuccess", tk.stats.batch_sigs_success);
    set_num(env, o, "deviceMs", tk.stats.device_ms);
    set_num(env, o, "workerStartNs", (double)t.t_start);
    set_num(env, o, "workerEndNs", (double)t.t_end);
    // lb_verify_requests_async returned / lb_wait called on it (0 after finish(): the call's two
    // halves were submitted apart)
    set_num(env, o, "workerSubmittedNs", one_phase ? (double)t.t_submitted : 0.0);
    set_num(env, o, "workerRetireNs", one_phase ? (double)t.t_retire : 0.0);
    return o;
  }
};
typedef std::map<uint64_t, std::unique_ptr<VerifyCall>> Partials;

struct VerifyTask : Task {
  VerifyCall call;
  bool submitted = false;
  uint64_t clk[4] = {};  // latency-lane calls: lb_last_latency_clocks
  // latency-lane calls with LB_STAGE_EVENTS=1: the call's stage times (lb_last_stage_times)
  float stage_ms[16] = {};
  const char* stage_names[16] = {};
  int n_stage = 0;

  int run(lb_ctx* ctx) override {
    const int rc = call.submit(ctx, prio ? VerifyCall::PRIORITY : VerifyCall::ASYNC);
    t_submitted = now_ns();
    submitted = rc == LB_OK;
    return rc;
  }
  Ticket* ticket() override { return submitted ? &call.tk : nullptr; }
  void read_lane_clocks(lb_ctx* lane) {
    lb_last_latency_clocks(lane, clk);
    n_stage = lb_last_stage_times(lane, stage_ms, stage_names, 16);
    if (n_stage > 16) n_stage = 16;
  }
  napi_value result(napi_env env) override {
    napi_value o = call.verdicts(env, *this, true);
    if (clk[2] > clk[0]) {  // latency lane: the kernel's own time and shader clock
      const double rt = (double)(clk[2] - clk[0]);
      set_num(env, o, "kernelMs", rt / 1e5);
      set_num(env, o, "kernelClockMHz", (double)(clk[3] - clk[1]) / rt * 100.0);
    }
    if (n_stage > 0) {
      napi_value st = make_object(env);
      for (int i = 0; i < n_stage; i++)
        if (stage_names[i]) set_num(env, st, stage_names[i], stage_ms[i]);
      set(env, o, "stageMs", st);
    }
    return o;
  }
};

// verifyRequestsPartial: resolves with the call's partial as soon as it is out; the call itself
// goes into the book, where finish(id) finds it
struct PartialTask : Task {
  std::unique_ptr<VerifyCall> call{new VerifyCall()};
  Partials* book = nullptr;
  uint64_t id = 0;
  std::vector<uint8_t> partial;

  int run(lb_ctx* ctx) override {
    call->t_start = t_start;
    partial.assign(LB_GT_BYTES, 0);
    int rc = call->submit(ctx, VerifyCall::PARTIAL);
    if (rc == LB_OK) rc = lb_partial_wait(ctx, call->tk.id, partial.data());
    if (rc != LB_OK) return rc;  // (the call and its inputs' references go with this task)
    call->refs.swap(refs);
    (*book)[id] = std::move(call);
    return LB_OK;
  }
  napi_value result(napi_env env) override {
    napi_value o = make_object(env);
    set_num(env, o, "id", (double)id);
    set(env, o, "partial", make_u8(env, partial.data(), LB_GT_BYTES));
    return o;
  }
};

// finish(id, mergedOk): takes the call out of the book, resumes it and is retired as that call
struct FinishTask : Task {
  Partials* book = nullptr;
  uint64_t id = 0;
  int merged_ok = 0;
  std::unique_ptr<VerifyCall> call;

  int run(lb_ctx* ctx) override {
    auto it = book->find(id);
    if (it == book->end()) return own_error(this, "unknown or already finished two-phase call");
    call = std::move(it->second);
    book->erase(it);
    t_start = call->t_start;
    refs.swap(call->refs);  // its inputs' references, released on the JS thread with this task
    // (a released call -- LB_TP_RELEASE, the default -- holds provisional verdicts until this
    // finish; a failed finish, e.g. the failed combine's re-run not submitted, rejects the
    // promise: the call still retires through lb_wait, whose error is kept)
    const int rc = lb_verify_requests_finish(ctx, call->tk.id, merged_ok);
    if (rc != LB_OK) fail(this, rc, ctx);
    return LB_OK;
  }
  Ticket* ticket() override { return call ? &call->tk : nullptr; }
  napi_value result(napi_env env) override { return call->verdicts(env, *this, false); }
};

// ---- verifySameMessage ------------------------------------------------------------------------
struct SameMessageTask : Task {
  uint32_t n_jobs = 0, n_sets = 0;
  std::vector<uint32_t> job_off, sig_off, pk_idx;
  std::vector<uint8_t> pubkeys, signatures, messages, seed;
  bool by_index = false, mixed = false;
  // {aggregate, mask}: the jobs' aggregate signatures as well
  bool agg = false, has_mask = false;
  std::vector<uint8_t> mask;
  std::vector<uint8_t> valid, job_fast, job_signatures;
  std::vector<uint32_t> job_counts;
  Ticket tk;
  bool submitted = false;

  int run(lb_ctx* ctx) override {
    lb_same_message_batch b{};
    b.n_jobs = n_jobs;
    b.n_sets = n_sets;
    b.job_offsets = job_off.data();
    b.pubkeys = (by_index && !mixed) ? nullptr : pubkeys.data();
    b.pubkey_indices = by_index ? pk_idx.data() : nullptr;
    b.signatures = signatures.data();
    b.sig_offsets = sig_off.data();
    b.messages = messages.data();
    b.seed = seed.data();
    alloc_out(valid, n_sets);
    alloc_out(job_fast, n_jobs);
    // in flight like a verify call (the package's per-set retries run when it retires)
    int rc;
    if (agg) {
      alloc_out(job_signatures, (size_t)n_jobs * LB_SIG_COMPRESSED);
      alloc_out(job_counts, n_jobs);
      rc = lb_verify_same_message_batch_agg_async(ctx, &b, has_mask ? mask.data() : nullptr, valid.data(),
                                                  job_fast.data(), job_signatures.data(), job_counts.data(), &tk.id);
    } else {
      rc = lb_verify_same_message_batch_async(ctx, &b, valid.data(), job_fast.data(), &tk.id);
    }
    submitted = rc == LB_OK;
    return rc;
  }
  Ticket* ticket() override { return submitted ? &tk : nullptr; }
  napi_value result(napi_env env) override {
    napi_value o = make_object(env);
    set(env, o, "valid", make_u8(env, valid.data(), n_sets));
    set(env, o, "jobFast", make_u8(env, job_fast.data(), n_jobs));
    set_num(env, o, "retriedJobs", tk.stats.batch_retries);
    set_num(env, o, "fastSets", tk.stats.batch_sigs_success);
    set_num(env, o, "deviceMs", tk.stats.device_ms);
    set_num(env, o, "workerStartNs", (double)t_start);
    set_num(env, o, "workerEndNs", (double)t_end);
    if (agg) {
      set(env, o, "jobSignatures", make_u8(env, job_signatures.data(), (size_t)n_jobs * LB_SIG_COMPRESSED));
      set(env, o, "jobCounts", make_u32s(env, job_counts, n_jobs));
    }
    return o;
  }
};

// ---- tables and lists: the lane's context follows each of them ------------------------------
struct SyncPubkeysTask : Task {
  std::vector<uint8_t> keys;
  uint32_t pk_len = 0, n_keys = 0;
  uint32_t size = 0;  // the table's, after the append

  int run(lb_ctx* ctx) override {
    int32_t bad = -1;
    const int rc = lb_pubkey_table_append(ctx, n_keys, keys.data(), pk_len, &bad);
    if (rc != LB_OK && bad >= 0) err_note = " (pubkey " + std::to_string(bad) + ")";
    if (rc == LB_OK) lb_pubkey_table_size(ctx, &size);
    return rc;
  }
  // (ctx's table, the authoritative one, already holds the keys: the task succeeds; a
  // lane that cannot follow is retired instead of left out of sync)
  const char* mirror_what() const override { return "pubkey table"; }
  int mirror(lb_ctx* lane) override {
    int32_t bad = -1;
    uint32_t n = 0;
    int rc = lb_pubkey_table_append(lane, n_keys, keys.data(), pk_len, &bad);
    if (rc == LB_OK) rc = lb_pubkey_table_size(lane, &n);
    return rc != LB_OK ? rc : n != size ? LB_ERR_DEVICE : LB_OK;
  }
  napi_value result(napi_env env) override { return make_uint(env, size); }
};

struct IndexListPutTask : Task {
  uint32_t list = 0, n = 0;
  std::vector<uint32_t> indices;

  int run(lb_ctx* ctx) override { return lb_index_list_put(ctx, list, n, indices.data()); }
  const char* mirror_what() const override { return "index lists"; }
  int mirror(lb_ctx* lane) override { return run(lane); }
  napi_value result(napi_env env) override { return make_uint(env, n); }
};

struct IndexListShuffleTask : Task {
  uint32_t list = 0, n = 0;
  std::vector<uint32_t> active;
  std::vector<uint8_t> seed;
  std::vector<uint32_t> shuffling;

  int run(lb_ctx* ctx) override {
    alloc_out(shuffling, n);
    return lb_index_list_shuffle(ctx, list, n, active.data(), seed.data(), shuffling.data());
  }
  // (the shuffling arrives at the lane computed)
  const char* mirror_what() const override { return "index lists"; }
  int mirror(lb_ctx* lane) override { return lb_index_list_put(lane, list, n, shuffling.data()); }
  napi_value result(napi_env env) override { return make_u32s(env, shuffling, n); }
};

struct BalancePutTask : Task {
  uint32_t first = 0, n = 0;
  std::vector<uint8_t> increments;
  uint32_t size = 0;  // the table's, after the put

  int run(lb_ctx* ctx) override {
    const int rc = lb_balance_table_put(ctx, first, n, increments.data());
    return rc != LB_OK ? rc : lb_balance_table_size(ctx, &size);
  }
  const char* mirror_what() const override { return "balance table"; }
  int mirror(lb_ctx* lane) override { return lb_balance_table_put(lane, first, n, increments.data()); }
  napi_value result(napi_env env) override { return make_uint(env, size); }
};

struct SampleTask : Task {
  std::vector<uint8_t> seeds;
  std::vector<uint32_t> active;
  uint32_t n_seeds = 0, n_active = 0, count = 0, max_increment = 0, max_candidates = 0;
  uint32_t store_list = LB_NO_LIST;  // the list a lone seed's filled committee replaces
  bool want_aggregate = false;       // and that list's aggregate key
  std::vector<uint32_t> indices, found, tried;
  bool stored = false, has_aggregate = false;
  std::vector<uint8_t> aggregate;

  int run(lb_ctx* ctx) override {
    alloc_out(indices, (size_t)n_seeds * count, LB_SAMPLE_NONE);
    alloc_out(found, n_seeds);
    alloc_out(tried, n_seeds);
    int rc = lb_sample_by_balance(ctx, n_seeds, seeds.data(), count, n_active, active.data(), max_increment,
                                  max_candidates, store_list, indices.data(), found.data(), tried.data());
    stored = rc == LB_OK && store_list != LB_NO_LIST && n_seeds == 1 && found[0] == count;
    if (stored && want_aggregate) {
      aggregate.assign(LB_PUBKEY_BYTES, 0);
      uint8_t st = 0;
      rc = lb_aggregate_pubkeys_list(ctx, store_list, 0, count, aggregate.data(), &st);
      has_aggregate = rc == LB_OK && st == LB_SET_OK;
      if (rc == LB_OK && st != LB_SET_OK) own_error(this, "invalid pubkey");  // (the list is stored: the lane follows)
    }
    return rc;
  }
  // (a committee follows only when it was stored; it arrives at the lane computed, as a shuffling does)
  const char* mirror_what() const override { return stored ? "index lists" : nullptr; }
  int mirror(lb_ctx* lane) override { return lb_index_list_put(lane, store_list, count, indices.data()); }
  napi_value result(napi_env env) override {
    napi_value o = make_object(env);
    set(env, o, "indices", make_u32s(env, indices, (size_t)n_seeds * count));
    set(env, o, "found", make_u32s(env, found, n_seeds));
    set(env, o, "tried", make_u32s(env, tried, n_seeds));
    if (has_aggregate) set(env, o, "aggregatePubkey", make_u8(env, aggregate.data(), LB_PUBKEY_BYTES));
    return o;
  }
};

// ---- aggregation, the combine's check ------------------------------------------------------------
struct AggPubkeysTask : Task {
  bool by_index = false;
  std::vector<uint32_t> indices;
  std::vector<uint8_t> keys;
  uint32_t n = 0;
  std::vector<uint8_t> aggregate;

  int run(lb_ctx* ctx) override {
    aggregate.assign(LB_PUBKEY_BYTES, 0);
    uint8_t st = 0;
    const int rc = by_index ? lb_aggregate_pubkeys_indexed(ctx, n, indices.data(), aggregate.data(), &st)
                            : lb_aggregate_pubkeys(ctx, n, keys.data(), aggregate.data(), &st);
    return rc != LB_OK || st == LB_SET_OK ? rc : own_error(this, "invalid pubkey");
  }
  napi_value result(napi_env env) override { return make_u8(env, aggregate.data(), LB_PUBKEY_BYTES); }
};

struct AggSigGroupsTask : Task {
  uint32_t n_groups = 0;
  std::vector<uint32_t> group_off, sig_off;
  std::vector<uint8_t> signatures;
  bool no_check = false;
  std::vector<uint8_t> group_signatures;
  std::vector<int32_t> bad_index;

  int run(lb_ctx* ctx) override {
    group_signatures.assign((size_t)n_groups * LB_SIG_COMPRESSED, 0);
    bad_index.assign(n_groups, -1);
    return lb_aggregate_signature_groups(ctx, n_groups, group_off.data(), signatures.data(), sig_off.data(),
                                         no_check ? LB_AGG_NO_CHECK : 0u, group_signatures.data(), bad_index.data());
  }
  napi_value result(napi_env env) override {
    napi_value o = make_object(env);
    set(env, o, "signatures", make_u8(env, group_signatures.data(), (size_t)n_groups * LB_SIG_COMPRESSED));
    set(env, o, "badIndex", make_words(env, napi_int32_array, bad_index.data(), n_groups));
    return o;
  }
};

struct GtCheckTask : Task {
  std::vector<uint8_t> partials;
  uint32_t n = 0;
  int32_t is_one = 0;

  int run(lb_ctx* ctx) override { return lb_gt_check(ctx, n, partials.data(), &is_one); }
  napi_value result(napi_env env) override { return make_bool(env, is_one != 0); }
};

// ---- KZG -------------------------------------------------------------------------------------
struct KzgLoadTask : Task {
  std::vector<uint8_t> g2_tau;
  int run(lb_ctx* ctx) override { return lb_kzg_load_setup(ctx, g2_tau.data()); }
  napi_value result(napi_env env) override { return make_undefined(env); }
};

struct KzgLoadG1Task : Task {
  std::vector<uint8_t> g1_lagrange;
  int run(lb_ctx* ctx) override {
    int32_t bad = -1;
    const int rc = lb_kzg_load_setup_g1(ctx, g1_lagrange.data(), &bad);
    if (rc != LB_OK && bad >= 0) err_note = " (bad index " + std::to_string(bad) + ")";
    return rc;
  }
  napi_value result(napi_env env) override { return make_undefined(env); }
};

struct KzgVerifyTask : Task {
  uint32_t n = 0;
  std::vector<uint8_t> blobs, commitments, proofs;
  int32_t ok = 0;
  std::vector<uint8_t> status;

  int run(lb_ctx* ctx) override {
    alloc_out(status, n);
    return lb_kzg_verify_blob_proof_batch(ctx, n, blobs.data(), commitments.data(), proofs.data(), &ok, status.data(),
                                          nullptr);
  }
  napi_value result(napi_env env) override {
    napi_value o = make_object(env);
    set(env, o, "ok", make_bool(env, ok != 0));
    set(env, o, "status", make_u8(env, status.data(), n));
    return o;
  }
};

// kzgBlobCommitments / kzgBlobProofs / kzgComputeProofs: n blobs in, 48 bytes and a status per blob out
// (an item with a status has all-zero outputs)
struct KzgBlobsTask : Task {
  uint32_t n = 0;
  std::vector<uint8_t> blobs;
  std::vector<uint8_t> out48, status;

  void alloc() {
    alloc_out(status, n);
    alloc_out(out48, (size_t)n * 48);
  }
  napi_value result_as(napi_env env, const char* out_name) {
    napi_value o = make_object(env);
    set(env, o, out_name, make_u8(env, out48.data(), (size_t)n * 48));
    return o;
  }
  napi_value with_status(napi_env env, napi_value o) {
    set(env, o, "status", make_u8(env, status.data(), n));
    return o;
  }
};
struct KzgCommitTask : KzgBlobsTask {
  int run(lb_ctx* ctx) override {
    alloc();
    return lb_kzg_blob_commitments(ctx, n, blobs.data(), out48.data(), status.data());
  }
  napi_value result(napi_env env) override { return with_status(env, result_as(env, "commitments")); }
};
struct KzgProveTask : KzgBlobsTask {
  std::vector<uint8_t> commitments;
  int run(lb_ctx* ctx) override {
    alloc();
    return lb_kzg_blob_proofs(ctx, n, blobs.data(), commitments.data(), out48.data(), status.data());
  }
  napi_value result(napi_env env) override { return with_status(env, result_as(env, "proofs")); }
};
struct KzgPointTask : KzgBlobsTask {
  std::vector<uint8_t> zs, ys;
  int run(lb_ctx* ctx) override {
    alloc();
    alloc_out(ys, (size_t)n * 32);
    return lb_kzg_compute_proofs(ctx, n, blobs.data(), zs.data(), out48.data(), ys.data(), status.data());
  }
  napi_value result(napi_env env) override {
    napi_value o = result_as(env, "proofs");
    set(env, o, "ys", make_u8(env, ys.data(), (size_t)n * 32));
    return with_status(env, o);
  }
};

// close(): the submission thread drains what is in flight and destroys both contexts (worker_loop)
struct CloseTask : Task {
  CloseTask() { close = true; }
  int run(lb_ctx*) override { return LB_OK; }
  napi_value result(napi_env env) override { return make_undefined(env); }
};

// ---- the per-GPU context ---------------------------------------------------------
struct Context {
  lb_ctx* ctx = nullptr;
  int device = 0;
  int capacity = 4;
  napi_env env = nullptr;
  napi_threadsafe_function tsfn = nullptr;
  std::thread worker;
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Task*> queue;
  bool closing = false;   // no new work accepted
  bool finalizing = false;
  bool joined = false;
  int pending = 0;        // JS thread only: tasks not yet completed
  uint64_t next_partial = 1;
  Partials partials;  // worker thread only: the two-phase calls between their partial and their finish
  // The latency lane (LB_PRIO_THREAD, default on): priority verify calls run on a context
  // of their own (lb_create_lane) driven by a thread of their own, so they never wait for
  // the submission thread's staging of throughput packages or its retiring of calls
  // (the reference's verifyOnMainThread / priority unshift,
  // BN/chain/bls/multithread/index.ts:174-187,544-555).  Its pubkey table, index lists and
  // balance table mirror ctx's (Task::mirror).
  lb_ctx* lctx = nullptr;
  // false once the lane's tables failed to follow ctx's: from then on
  // priority calls go back to ctx (the submission thread), never to a table that resolves
  // indices differently
  std::atomic<bool> lane_ok{true};
  std::thread lane;
  std::mutex lmu;
  std::condition_variable lcv;
  std::deque<Task*> lqueue;
  bool lane_stop = false;
};

void complete(Context* c, Task* t) {
  if (c->finalizing) {
    delete t;
    return;
  }
  napi_call_threadsafe_function(c->tsfn, t, napi_tsfn_blocking);
}

// Into the submission thread's queue (c->mu held): a priority task ahead of every queued
// non-priority task, behind earlier priority ones
void enqueue(Context* c, Task* t) {
  auto it = c->queue.end();
  if (t->prio) {
    it = c->queue.begin();
    while (it != c->queue.end() && (*it)->prio) ++it;
  }
  c->queue.insert(it, t);
}

void hand_to_lane(Context* c, Task* t) {
  {
    std::lock_guard<std::mutex> lk(c->lmu);
    c->lqueue.push_back(t);
  }
  c->lcv.notify_one();
}

// The lane's context follows ctx (which already holds what t put there: the task succeeds); a
// lane that cannot follow is retired instead of left out of sync
void follow(Context* c, Task* t) {
  if (!c->lane_ok || t->mirror(c->lctx) == LB_OK) return;
  c->lane_ok = false;
  fprintf(stderr, "lodestar_bls: latency lane retired (its %s could not follow: %s); priority calls run on "
                  "the main context\n", t->mirror_what(), lb_last_error(c->lctx));
}

// The lane thread: owns c->lctx.  Priority verify calls one at a time (the priority slot
// admits one), and the second half of every mirrored operation (the main worker runs it
// on ctx first, then hands the task here).
void lane_loop(Context* c) {
  for (;;) {
    Task* t = nullptr;
    {
      std::unique_lock<std::mutex> lk(c->lmu);
      c->lcv.wait(lk, [&] { return !c->lqueue.empty() || c->lane_stop; });
      if (c->lqueue.empty()) break;  // stopped and drained
      t = c->lqueue.front();
      c->lqueue.pop_front();
    }
    if (c->finalizing) {
      delete t;
      continue;
    }
    if (t->mirror_what()) {
      follow(c, t);
      complete(c, t);
      continue;
    }
    if (!c->lane_ok) {  // a priority call queued here before the lane retired: back to ctx
      {
        std::lock_guard<std::mutex> lk(c->mu);
        enqueue(c, t);
      }
      c->cv.notify_all();
      continue;
    }
    VerifyTask* v = static_cast<VerifyTask*>(t);  // (submit() sends nothing else here)
    v->t_start = now_ns();
    int rc = v->run(c->lctx);
    if (rc == LB_OK) {
      v->t_retire = now_ns();
      rc = lb_wait(c->lctx, v->call.tk.id, &v->call.tk.stats);
      if (rc == LB_OK) v->read_lane_clocks(c->lctx);
    }
    if (rc != LB_OK) fail(v, rc, c->lctx);
    v->t_end = now_ns();
    complete(c, v);
  }
  lb_destroy(c->lctx);
  c->lctx = nullptr;
}

// stop the lane thread after it has drained its queue (worker thread, before lb_destroy)
void lane_join(Context* c) {
  if (!c->lane.joinable()) return;
  {
    std::lock_guard<std::mutex> lk(c->lmu);
    c->lane_stop = true;
  }
  c->lcv.notify_one();
  c->lane.join();
}

// A queued task the worker can start now: a priority call always (its lane is
// separate from the calls in flight), close always, anything else when a slot is free.
bool startable(Context* c, size_t n_inflight) {
  if (c->queue.empty()) return false;
  const Task* f = c->queue.front();
  return f->prio || f->close || (int)n_inflight < c->capacity;
}

// lb_poll on a task in flight: 1 when lb_wait would return at once, 0 while it runs, -1 when
// the poll itself failed
int polled(Context* c, Task* w) {
  int32_t done = 0;
  return lb_poll(c->ctx, w->ticket()->id, &done) != LB_OK ? -1 : done ? 1 : 0;
}

// Wait for a task in flight (by now without blocking, except in close and the finalizer),
// take its stats and complete it.
void retire(Context* c, Task* w) {
  Ticket* k = w->ticket();
  w->t_retire = now_ns();
  const int rc = lb_wait(c->ctx, k->id, &k->stats);
  if (rc != LB_OK) fail(w, rc, c->ctx);
  w->t_end = now_ns();
  complete(c, w);
}

// Worker thread: owns c->ctx.
void worker_loop(Context* c) {
  std::deque<Task*> inflight;  // submitted, waiting for lb_wait
  std::deque<Task*> prio;      // priority-lane calls in flight (retired as soon as done)
  // a finished priority call retires ahead of everything
  const auto retire_prio = [&](bool unpolled) {
    if (prio.empty() || !(unpolled || polled(c, prio.front()) == 1)) return false;
    Task* w = prio.front();
    prio.pop_front();
    retire(c, w);
    return true;
  };
  Task* closing = nullptr;
  for (;;) {
    Task* t = nullptr;
    // ... before anything else is started: with packages startable back to back (each ~3 ms of
    // staging in lb_verify_requests_async), its verdict would otherwise wait behind all of them
    if (retire_prio(false)) continue;
    {
      std::unique_lock<std::mutex> lk(c->mu);
      c->cv.wait(lk, [&] { return !c->queue.empty() || !inflight.empty() || !prio.empty() || c->finalizing; });
      if (startable(c, inflight.size())) {
        t = c->queue.front();
        c->queue.pop_front();
      } else if (inflight.empty() && prio.empty() && c->finalizing) {
        break;
      }
    }
    if (!t && !prio.empty()) {
      if (retire_prio(c->finalizing)) continue;
      if (inflight.empty()) {
        std::unique_lock<std::mutex> lk(c->mu);
        c->cv.wait_for(lk, std::chrono::microseconds(50), [&] { return startable(c, 0) || c->finalizing; });
        continue;
      }
    }
    if (!t) {  // retire the oldest call in flight
      Task* w = inflight.front();
      // never block on it: the JS thread may queue the next package (blocking here held
      // every new package back until the oldest call finished: ~12 of 16 calls in
      // flight, 2.3 M sets/s through node), or a priority call that must start now
      if (!c->finalizing && polled(c, w) == 0) {
        std::unique_lock<std::mutex> lk(c->mu);
        c->cv.wait_for(lk, std::chrono::microseconds(prio.empty() ? 200 : 50),
                       [&] { return startable(c, inflight.size()) || c->finalizing; });
        continue;
      }
      inflight.pop_front();
      retire(c, w);
      continue;
    }
    if (t->close) {
      closing = t;
      break;
    }
    t->t_start = now_ns();
    const int rc = t->run(c->ctx);
    if (rc != LB_OK) fail(t, rc, c->ctx);
    if (rc == LB_OK && t->ticket()) {
      (t->prio ? prio : inflight).push_back(t);
    } else if (rc == LB_OK && t->mirror_what() && c->lctx && c->lane_ok) {
      hand_to_lane(c, t);  // the same into the latency lane's context, then resolve
    } else {
      t->t_end = now_ns();
      complete(c, t);
    }
  }
  // close(), or the finalizer (Context garbage-collected without close(): complete() deletes).
  // Never destroy the context under a call in flight; two-phase calls never finished go with it;
  // the lane's queued tasks complete before its context goes, and ctx goes last.
  while (retire_prio(true)) {
  }
  for (; !inflight.empty(); inflight.pop_front()) retire(c, inflight.front());
  c->partials.clear();
  lane_join(c);
  lb_destroy(c->ctx);
  c->ctx = nullptr;
  if (closing) complete(c, closing);
}

// ---- JS side -----------------------------------------------------------------------
void call_js(napi_env env, napi_value /*cb*/, void* context, void* data) {
  Context* c = static_cast<Context*>(context);
  Task* t = static_cast<Task*>(data);
  if (env == nullptr) {  // environment tearing down
    delete t;
    return;
  }
  release_refs(env, t->refs);
  if (t->rc != LB_OK)
    napi_reject_deferred(env, t->deferred, make_error(env, t->rc, t->errmsg));
  else
    napi_resolve_deferred(env, t->deferred, t->result(env));
  const bool closed = t->close;
  delete t;
  if (--c->pending == 0 && !closed) napi_unref_threadsafe_function(env, c->tsfn);
  if (closed) {
    if (c->worker.joinable()) c->worker.join();
    c->joined = true;
    napi_release_threadsafe_function(c->tsfn, napi_tsfn_release);
    c->tsfn = nullptr;
  }
}

Context* unwrap(napi_env env, napi_callback_info info, size_t* argc, napi_value* argv) {
  napi_value self;
  napi_get_cb_info(env, info, argc, argv, &self, nullptr);
  void* p = nullptr;
  napi_unwrap(env, self, &p);
  return static_cast<Context*>(p);
}

// Queue a task; returns its promise (rejected at once when the context is closed).
napi_value submit(napi_env env, Context* c, Task* t) {
  napi_value promise;
  napi_create_promise(env, &t->deferred, &promise);
  {
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->closing) {
      napi_reject_deferred(env, t->deferred, make_error(env, LB_ERR_INVALID_ARGUMENT, "QUEUE_ERROR_QUEUE_ABORTED: context closed"));
      release_refs(env, t->refs);
      delete t;
      return promise;
    }
    if (t->close) c->closing = true;
    if (t->prio && c->lctx && c->lane_ok) {
      // the latency lane: its own thread and context; the throughput context's calls
      // submitted from now on leave the reserved CUs free (lb_mark_priority)
      lb_mark_priority(c->ctx);
      if (c->pending++ == 0) napi_ref_threadsafe_function(env, c->tsfn);
      hand_to_lane(c, t);
      return promise;
    }
    enqueue(c, t);
  }
  if (c->pending++ == 0) napi_ref_threadsafe_function(env, c->tsfn);
  c->cv.notify_one();
  return promise;
}

napi_value rejected(napi_env env, const std::string& msg) {
  napi_deferred d;
  napi_value promise, m, e;
  napi_create_promise(env, &d, &promise);
  napi_create_string_utf8(env, msg.c_str(), NAPI_AUTO_LENGTH, &m);
  napi_create_type_error(env, nullptr, m, &e);
  napi_reject_deferred(env, d, e);
  return promise;
}

// The frame of every method: a T, filled by parse(t, context, argc, argv) from at least
// min_args arguments (an ArgError rejects the promise with a TypeError), then queued.
template <class T, class Parse>
napi_value method(napi_env env, napi_callback_info info, const char* usage, size_t min_args, Parse parse) {
  size_t argc = 3;
  napi_value argv[3];
  Context* c = unwrap(env, info, &argc, argv);
  if (!c || argc < min_args) return rejected(env, usage);
  std::unique_ptr<T> t(new T());
  try {
    parse(*t, *c, argc, argv);
  } catch (const ArgError& e) {
    release_refs(env, t->refs);
    return rejected(env, e.msg);
  }
  return submit(env, c, t.release());
}

napi_value VerifyRequests(napi_env env, napi_callback_info info) {
  return method<VerifyTask>(env, info, "verifyRequests(batch[, {priority}])", 1,
                            [&](VerifyTask& t, Context&, size_t argc, napi_value* argv) {
                              parse_requests(env, argv[0], t.call.in, t.refs);
                              opt_bool(env, argc, argv, 1, "priority", &t.prio);
                            });
}

napi_value VerifyRequestsPartial(napi_env env, napi_callback_info info) {
  return method<PartialTask>(env, info, "verifyRequests(batch[, {priority}])", 1,
                             [&](PartialTask& t, Context& c, size_t, napi_value* argv) {
                               parse_requests(env, argv[0], t.call->in, t.refs);
                               t.book = &c.partials;
                               t.id = c.next_partial++;
                             });
}

napi_value Finish(napi_env env, napi_callback_info info) {
  return method<FinishTask>(env, info, "finish(id, mergedOk)", 2, [&](FinishTask& t, Context& c, size_t, napi_value* argv) {
    double id = 0;
    bool ok = false;
    if (napi_get_value_double(env, argv[0], &id) != napi_ok || napi_get_value_bool(env, argv[1], &ok) != napi_ok)
      throw ArgError{"finish(id: number, mergedOk: boolean)"};
    t.book = &c.partials;
    t.id = (uint64_t)id;
    t.merged_ok = ok ? 1 : 0;
  });
}

napi_value GtCheck(napi_env env, napi_callback_info info) {
  return method<GtCheckTask>(env, info, "gtCheck(partials: Uint8Array)", 1,
                             [&](GtCheckTask& t, Context&, size_t, napi_value* argv) {
                               typed(env, argv[0], napi_uint8_array, "partials", t.partials);
                               if (t.partials.size() % LB_GT_BYTES) throw ArgError{"partials: 576 bytes each"};
                               t.n = (uint32_t)(t.partials.size() / LB_GT_BYTES);
                               pad(t.partials);
                             });
}

napi_value VerifySameMessage(napi_env env, napi_callback_info info) {
  return method<SameMessageTask>(env, info, "verifySameMessage(batch)", 1,
                                 [&](SameMessageTask& t, Context&, size_t argc, napi_value* argv) {
    napi_value o = argv[0], seedv;
    req_typed(env, o, "jobOffsets", napi_uint32_array, t.job_off);
    if (t.job_off.empty()) throw ArgError{"jobOffsets: wrong length"};
    t.n_jobs = (uint32_t)t.job_off.size() - 1;
    t.n_sets = t.job_off.back();
    check_offsets(t.job_off, t.n_jobs, UINT32_MAX, "jobOffsets");
    req_typed(env, o, "signatures", napi_uint8_array, t.signatures);
    req_typed(env, o, "sigOffsets", napi_uint32_array, t.sig_off);
    check_offsets(t.sig_off, t.n_sets, (uint32_t)t.signatures.size(), "sigOffsets");
    req_typed(env, o, "messages", napi_uint8_array, t.messages);
    if (t.messages.size() != (size_t)t.n_jobs * 32) throw ArgError{"messages: 32 bytes per job"};
    if (!has_prop(env, o, "seed", &seedv)) throw ArgError{"missing seed"};
    seed32(env, seedv, t.seed);
    t.by_index = opt_typed(env, o, "pubkeyIndices", napi_uint32_array, t.pk_idx);
    if (t.by_index) {
      if (t.pk_idx.size() != t.n_sets) throw ArgError{"pubkeyIndices: one per set"};
      t.mixed = opt_typed(env, o, "pubkeys", napi_uint8_array, t.pubkeys);
      check_pk_rows(t.pk_idx.data(), t.pk_idx.size(), t.mixed, t.pubkeys.size());
    } else {
      if (!opt_typed(env, o, "pubkeys", napi_uint8_array, t.pubkeys) && t.n_sets)
        throw ArgError{"missing pubkeys (or pubkeyIndices)"};
      if (t.pubkeys.size() != (size_t)t.n_sets * LB_PUBKEY_BYTES) throw ArgError{"pubkeys: 96 bytes per set"};
    }
    pad(t.signatures);
    pad(t.messages);
    pad(t.pubkeys);
    pad(t.pk_idx);
    // {aggregate: true, mask?}: the jobs' aggregate signatures as well; without it nothing changes
    opt_bool(env, argc, argv, 1, "aggregate", &t.agg);
    if (t.agg) {
      t.has_mask = opt_typed(env, argv[1], "mask", napi_uint8_array, t.mask);
      if (t.has_mask && t.mask.size() != t.n_sets) throw ArgError{"mask: one byte per set"};
      pad(t.mask);
    }
  });
}

napi_value AggregateSignatureGroups(napi_env env, napi_callback_info info) {
  return method<AggSigGroupsTask>(
      env, info, "aggregateSignatureGroups({groupOffsets, signatures, sigOffsets}, {noCheck?})", 1,
      [&](AggSigGroupsTask& t, Context&, size_t argc, napi_value* argv) {
        napi_value o = argv[0];
        req_typed(env, o, "groupOffsets", napi_uint32_array, t.group_off);
        if (t.group_off.size() < 2) throw ArgError{"EMPTY_AGGREGATE_ARRAY"};
        t.n_groups = (uint32_t)t.group_off.size() - 1;
        check_offsets(t.group_off, t.n_groups, UINT32_MAX, "groupOffsets");
        for (uint32_t g = 0; g < t.n_groups; g++)
          if (t.group_off[g + 1] == t.group_off[g]) throw ArgError{"EMPTY_AGGREGATE_ARRAY"};
        req_typed(env, o, "signatures", napi_uint8_array, t.signatures);
        req_typed(env, o, "sigOffsets", napi_uint32_array, t.sig_off);
        check_offsets(t.sig_off, t.group_off.back(), (uint32_t)t.signatures.size(), "sigOffsets");
        pad(t.signatures);
        opt_bool(env, argc, argv, 1, "noCheck", &t.no_check);
      });
}

napi_value SyncPubkeys(napi_env env, napi_callback_info info) {
  return method<SyncPubkeysTask>(env, info, "syncPubkeys(keys: Uint8Array, pkLen: 48 | 96)", 2,
                                 [&](SyncPubkeysTask& t, Context&, size_t, napi_value* argv) {
                                   typed(env, argv[0], napi_uint8_array, "keys", t.keys);
                                   napi_get_value_uint32(env, argv[1], &t.pk_len);
                                   if (t.pk_len != 48 && t.pk_len != 96) throw ArgError{"pkLen must be 48 or 96"};
                                   if (t.keys.size() % t.pk_len) throw ArgError{"keys: a whole number of keys"};
                                   t.n_keys = (uint32_t)(t.keys.size() / t.pk_len);
                                   pad(t.keys);
                                 });
}

uint32_t list_id(napi_env env, napi_value v) {
  uint32_t id = 0;
  if (napi_get_value_uint32(env, v, &id) != napi_ok) throw ArgError{"listId must be a number"};
  return id;
}
napi_value IndexListPut(napi_env env, napi_callback_info info) {
  return method<IndexListPutTask>(env, info, "indexListPut(listId, indices: Uint32Array)", 2,
                                  [&](IndexListPutTask& t, Context&, size_t, napi_value* argv) {
                                    t.list = list_id(env, argv[0]);
                                    typed(env, argv[1], napi_uint32_array, "indices", t.indices);
                                    t.n = (uint32_t)t.indices.size();
                                    pad(t.indices);
                                  });
}
napi_value IndexListShuffle(napi_env env, napi_callback_info info) {
  return method<IndexListShuffleTask>(env, info, "indexListShuffle(listId, activeIndices: Uint32Array, seed: Uint8Array)", 3,
                                      [&](IndexListShuffleTask& t, Context&, size_t, napi_value* argv) {
                                        t.list = list_id(env, argv[0]);
                                        typed(env, argv[1], napi_uint32_array, "indices", t.active);
                                        t.n = (uint32_t)t.active.size();
                                        pad(t.active);
                                        seed32(env, argv[2], t.seed);
                                      });
}

napi_value BalanceTablePut(napi_env env, napi_callback_info info) {
  return method<BalancePutTask>(env, info, "balanceTablePut(first, increments: Uint8Array)", 2,
                                [&](BalancePutTask& t, Context&, size_t, napi_value* argv) {
                                  if (napi_get_value_uint32(env, argv[0], &t.first) != napi_ok)
                                    throw ArgError{"first must be a number"};
                                  typed(env, argv[1], napi_uint8_array, "increments", t.increments);
                                  t.n = (uint32_t)t.increments.size();
                                  pad(t.increments);
                                });
}

napi_value SampleByBalance(napi_env env, napi_callback_info info) {
  const char* usage = "sampleByBalance({seeds, count, activeIndices, maxIncrement, maxCandidates, storeList?, aggregate?})";
  return method<SampleTask>(env, info, usage, 1, [&](SampleTask& t, Context&, size_t, napi_value* argv) {
    if (!is_object(env, argv[0])) throw ArgError{usage};
    napi_value o = argv[0], v;
    req_typed(env, o, "seeds", napi_uint8_array, t.seeds);
    if (t.seeds.size() % 32) throw ArgError{"seeds: 32 bytes each"};
    t.n_seeds = (uint32_t)(t.seeds.size() / 32);
    pad(t.seeds);
    req_typed(env, o, "activeIndices", napi_uint32_array, t.active);
    t.n_active = (uint32_t)t.active.size();
    pad(t.active);
    const auto num = [&](const char* name, uint32_t* out) {
      if (!has_prop(env, o, name, &v) || napi_get_value_uint32(env, v, out) != napi_ok)
        throw ArgError{std::string(name) + " must be a number"};
    };
    num("count", &t.count);
    num("maxIncrement", &t.max_increment);
    num("maxCandidates", &t.max_candidates);
    if (has_prop(env, o, "storeList", &v) && napi_get_value_uint32(env, v, &t.store_list) != napi_ok)
      throw ArgError{"storeList must be a number"};
    if (has_prop(env, o, "aggregate", &v)) napi_get_value_bool(env, v, &t.want_aggregate);
    // (the output is sized here: the library's own limits refuse anything larger)
    if (t.count > LB_SAMPLE_MAX_COUNT) throw ArgError{"count above LB_SAMPLE_MAX_COUNT"};
    if (t.n_seeds > LB_SAMPLE_MAX_SEEDS) throw ArgError{"more than LB_SAMPLE_MAX_SEEDS seeds"};
  });
}

napi_value AggregatePubkeys(napi_env env, napi_callback_info info) {
  return method<AggPubkeysTask>(env, info, "aggregatePubkeys(keys: Uint8Array | indices: Uint32Array)", 1,
                                [&](AggPubkeysTask& t, Context&, size_t, napi_value* argv) {
    bool is = false;
    napi_is_typedarray(env, argv[0], &is);
    if (!is) throw ArgError{"aggregatePubkeys expects a typed array"};
    t.by_index = array_info(env, argv[0], "keys").type == napi_uint32_array;
    if (t.by_index) {
      typed(env, argv[0], napi_uint32_array, "indices", t.indices);
      t.n = (uint32_t)t.indices.size();
    } else {
      typed(env, argv[0], napi_uint8_array, "keys", t.keys);
      if (t.keys.size() % LB_PUBKEY_BYTES) throw ArgError{"keys: 96 bytes each"};
      t.n = (uint32_t)(t.keys.size() / LB_PUBKEY_BYTES);
    }
    if (t.n == 0) throw ArgError{"EMPTY_AGGREGATE_ARRAY"};
  });
}

// kzgLoadSetup(g2Tau: Uint8Array(96)): KZG_SETUP_G2_MONOMIAL[1], compressed
napi_value KzgLoadSetup(napi_env env, napi_callback_info info) {
  return method<KzgLoadTask>(env, info, "kzgLoadSetup(g2Tau: Uint8Array(96))", 1,
                             [&](KzgLoadTask& t, Context&, size_t, napi_value* argv) {
                               typed(env, argv[0], napi_uint8_array, "g2Tau", t.g2_tau);
                               if (t.g2_tau.size() != 96) throw ArgError{"g2Tau: 96 bytes"};
                             });
}

// kzgLoadSetupG1(g1Lagrange: Uint8Array(4096 x 48)): the G1 lines of trusted_setup.txt, file order; a
// refused point rejects with its index in the message
napi_value KzgLoadSetupG1(napi_env env, napi_callback_info info) {
  return method<KzgLoadG1Task>(env, info, "kzgLoadSetupG1(g1Lagrange: Uint8Array(196608))", 1,
                               [&](KzgLoadG1Task& t, Context&, size_t, napi_value* argv) {
                                 typed(env, argv[0], napi_uint8_array, "g1Lagrange", t.g1_lagrange);
                                 if (t.g1_lagrange.size() != 4096 * 48) throw ArgError{"g1Lagrange: 196608 bytes"};
                               });
}

// kzgVerifyBlobProofBatch(blobs: n x 131072, commitments: n x 48, proofs: n x 48)
//   -> Promise<{ok: boolean, status: Uint8Array(n)}>   (status: LB_KZG_*; ok is false when any is set)
napi_value KzgVerifyBlobProofBatch(napi_env env, napi_callback_info info) {
  return method<KzgVerifyTask>(env, info, "kzgVerifyBlobProofBatch(blobs, commitments, proofs: Uint8Array)", 3,
                               [&](KzgVerifyTask& t, Context&, size_t, napi_value* argv) {
    t.n = parse_blobs(env, argv[0], t.blobs);
    parse_per_blob(env, argv[1], "commitments", 48, t.n, "commitments: 48 bytes per blob", t.commitments);
    parse_per_blob(env, argv[2], "proofs", 48, t.n, "proofs: 48 bytes per blob", t.proofs);
  });
}

// kzgBlobCommitments(blobs) / kzgBlobProofs(blobs, commitments: n x 48) / kzgComputeProofs(blobs, zs: n x 32)
//   -> Promise<{commitments | proofs: Uint8Array(n x 48), [ys: Uint8Array(n x 32),] status: Uint8Array(n)}>
napi_value KzgBlobCommitments(napi_env env, napi_callback_info info) {
  return method<KzgCommitTask>(env, info, "kzgBlobCommitments(blobs: Uint8Array)", 1,
                               [&](KzgCommitTask& t, Context&, size_t, napi_value* argv) {
                                 t.n = parse_blobs(env, argv[0], t.blobs);
                               });
}
napi_value KzgBlobProofs(napi_env env, napi_callback_info info) {
  return method<KzgProveTask>(env, info, "kzgBlobProofs(blobs, commitments: Uint8Array)", 2,
                              [&](KzgProveTask& t, Context&, size_t, napi_value* argv) {
    t.n = parse_blobs(env, argv[0], t.blobs);
    parse_per_blob(env, argv[1], "commitments", 48, t.n, "commitments: 48 bytes per blob", t.commitments);
  });
}
napi_value KzgComputeProofs(napi_env env, napi_callback_info info) {
  return method<KzgPointTask>(env, info, "kzgComputeProofs(blobs, zs: Uint8Array)", 2,
                              [&](KzgPointTask& t, Context&, size_t, napi_value* argv) {
    t.n = parse_blobs(env, argv[0], t.blobs);
    parse_per_blob(env, argv[1], "zs", 32, t.n, "zs: 32 bytes per blob", t.zs);
  });
}

napi_value Close(napi_env env, napi_callback_info info) {
  size_t argc = 0;
  Context* c = unwrap(env, info, &argc, nullptr);
  if (!c) return rejected(env, "not a Context");
  {
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->closing) {  // second close(): already resolved or pending
      napi_deferred d;
      napi_value p;
      napi_create_promise(env, &d, &p);
      napi_resolve_deferred(env, d, make_undefined(env));
      return p;
    }
  }
  return submit(env, c, new CloseTask());
}

void finalize_ctx(napi_env env, void* data, void* /*hint*/) {
  Context* c = static_cast<Context*>(data);
  if (!c->joined) {
    const auto drop = [&](std::mutex& mu, std::deque<Task*>& q) {
      std::lock_guard<std::mutex> lk(mu);
      c->finalizing = c->closing = true;
      for (Task* t : q) {
        release_refs(env, t->refs);
        delete t;
      }
      q.clear();
    };
    drop(c->mu, c->queue);
    drop(c->lmu, c->lqueue);
    c->cv.notify_one();
    if (c->worker.joinable()) c->worker.join();
    if (c->tsfn) napi_release_threadsafe_function(c->tsfn, napi_tsfn_abort);
  }
  delete c;
}

napi_value New(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2], self;
  napi_get_cb_info(env, info, &argc, argv, &self, nullptr);
  int32_t device = 0;
  if (argc >= 1) napi_get_value_int32(env, argv[0], &device);
  int32_t capacity = 0;  // default: the library's calls in flight (lb_slots)
  napi_value v;
  if (argc >= 2 && has_prop(env, argv[1], "capacity", &v)) napi_get_value_int32(env, v, &capacity);
  // sameMessageRandomized: true -> same-message jobs aggregated with per-set random scalars
  // (LB_SM_RANDOMIZED) on every context created here; absent / false -> the library's initial
  // mode (plain sums, or the operator's LB_SM_RANDOMIZED=1)
  bool sm_randomized = false;
  if (argc >= 2 && has_prop(env, argv[1], "sameMessageRandomized", &v)) napi_get_value_bool(env, v, &sm_randomized);
  lb_ctx* ctx = nullptr;
  const int rc = lb_create(device, &ctx);
  if (rc != LB_OK) {
    napi_throw(env, make_error(env, rc, "lb_create(" + std::to_string(device) + ") failed: " + lb_last_error(nullptr)));
    return nullptr;
  }
  if (capacity <= 0) capacity = lb_slots(ctx);
  Context* c = new Context();
  c->ctx = ctx;
  c->device = device;
  c->capacity = capacity < 1 ? 1 : capacity;
  c->env = env;
  {
    const char* e = getenv("LB_PRIO_THREAD");
    if (!(e && atoi(e) == 0) && lb_create_lane(device, &c->lctx) != LB_OK) c->lctx = nullptr;  // (then: no lane)
  }
  if (sm_randomized) {  // before any call: the main context and the latency lane's alike
    lb_set_same_message_mode(c->ctx, LB_SM_RANDOMIZED);
    if (c->lctx) lb_set_same_message_mode(c->lctx, LB_SM_RANDOMIZED);
  }
  napi_value name;
  napi_create_string_utf8(env, "lodestar_bls_gpu", NAPI_AUTO_LENGTH, &name);
  napi_create_threadsafe_function(env, nullptr, nullptr, name, 0, 1, nullptr, nullptr, c, call_js, &c->tsfn);
  napi_unref_threadsafe_function(env, c->tsfn);  // idle contexts do not keep the process alive
  c->worker = std::thread(worker_loop, c);
  if (c->lctx) c->lane = std::thread(lane_loop, c);
  napi_wrap(env, self, c, finalize_ctx, nullptr, nullptr);
  napi_value dev, cap;
  napi_create_int32(env, device, &dev);
  napi_set_named_property(env, self, "device", dev);
  napi_create_int32(env, c->capacity, &cap);
  napi_set_named_property(env, self, "capacity", cap);
  // the mode in force (the option, or the library's initial mode)
  set(env, self, "sameMessageRandomized", make_bool(env, lb_same_message_mode(c->ctx) == (int)LB_SM_RANDOMIZED));
  return self;
}

napi_value DeviceCount(napi_env env, napi_callback_info) {
  napi_value r;
  napi_create_int32(env, lb_device_count(), &r);
  return r;
}

// Marshalling dry run (no device): the same checks verifyRequests applies.
napi_value ValidateRequests(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  Requests r;
  std::vector<napi_ref> refs;
  try {
    if (argc < 1) throw ArgError{"validateRequests(batch)"};
    parse_requests(env, argv[0], r, refs);
  } catch (const ArgError& e) {
    release_refs(env, refs);
    napi_throw_type_error(env, nullptr, e.msg.c_str());
    return nullptr;
  }
  release_refs(env, refs);
  napi_value o = make_object(env);
  set_num(env, o, "nRequests", r.n_req);
  set_num(env, o, "nSets", r.n_sets);
  set_num(env, o, "nPubkeys", (double)r.n_pubkeys());
  set(env, o, "byIndex", make_bool(env, r.by_index));
  return o;
}

napi_value Init(napi_env env, napi_value exports) {
  // 16 HIP hardware queues for this process: the library keeps one call in flight per
  // queue (lb_slots), 3.03 vs 2.74 M sets/s over HIP's default 4 (profiles/ab_r03/hwq2).
  // Before the first HIP call (lb_create).  A GPU_MAX_HW_QUEUES the host already set
  // wins; LB_HW_QUEUES picks another count, clamped to [1, 16] -- lb_create refuses
  // more (each queue reserves scratch for the largest private segment).
  int nq = 16;
  if (const char* q = getenv("LB_HW_QUEUES")) nq = atoi(q) < 1 ? 1 : atoi(q) > 16 ? 16 : atoi(q);
  char qs[8];
  snprintf(qs, sizeof qs, "%d", nq);
  setenv("GPU_MAX_HW_QUEUES", qs, 0);
  // no per-stage timing events in the library (nothing on the JS side reads them; they
  // are two HIP calls per kernel on the submission thread); LB_STAGE_EVENTS=1 keeps them
  setenv("LB_STAGE_EVENTS", "0", 0);
  napi_property_descriptor methods[] = {
      {"verifyRequests", nullptr, VerifyRequests, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"verifyRequestsPartial", nullptr, VerifyRequestsPartial, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"finish", nullptr, Finish, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"gtCheck", nullptr, GtCheck, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"verifySameMessage", nullptr, VerifySameMessage, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"syncPubkeys", nullptr, SyncPubkeys, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"indexListPut", nullptr, IndexListPut, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"indexListShuffle", nullptr, IndexListShuffle, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"balanceTablePut", nullptr, BalanceTablePut, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"sampleByBalance", nullptr, SampleByBalance, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"aggregatePubkeys", nullptr, AggregatePubkeys, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"aggregateSignatureGroups", nullptr, AggregateSignatureGroups, nullptr, nullptr, nullptr, napi_default,
       nullptr},
      {"kzgLoadSetup", nullptr, KzgLoadSetup, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"kzgLoadSetupG1", nullptr, KzgLoadSetupG1, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"kzgBlobCommitments", nullptr, KzgBlobCommitments, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"kzgBlobProofs", nullptr, KzgBlobProofs, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"kzgComputeProofs", nullptr, KzgComputeProofs, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"kzgVerifyBlobProofBatch", nullptr, KzgVerifyBlobProofBatch, nullptr, nullptr, nullptr, napi_default,
       nullptr},
      {"close", nullptr, Close, nullptr, nullptr, nullptr, napi_default, nullptr},
  };
  napi_value cls;
  napi_define_class(env, "Context", NAPI_AUTO_LENGTH, New, nullptr, sizeof(methods) / sizeof(methods[0]), methods,
                    &cls);
  napi_set_named_property(env, exports, "Context", cls);
  napi_value f;
  napi_create_function(env, "deviceCount", NAPI_AUTO_LENGTH, DeviceCount, nullptr, &f);
  napi_set_named_property(env, exports, "deviceCount", f);
  napi_create_function(env, "validateRequests", NAPI_AUTO_LENGTH, ValidateRequests, nullptr, &f);
  napi_set_named_property(env, exports, "validateRequests", f);
  napi_value sz;
  napi_create_int32(env, LB_GT_BYTES, &sz);
  napi_set_named_property(env, exports, "GT_BYTES", sz);
  return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
