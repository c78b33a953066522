/* A stand-in for liblodestar_bls.so: exactly the lb_* entry points napi/addon.cc references, with
 * no device behind them, so the addon's scheduling (priority order, the capacity bound, mirroring
 * into the latency lane, lane retirement, partial -> finish, close) runs under node on a CPU
 * (tests/js/addon_sched.js).
 *
 * Every call on a context appends one line to the file LB_STUB_LOG named when the context was
 * created: "<ctx> <function> key=value ...", <ctx> being "main" (lb_create) or "lane"
 * (lb_create_lane); a call on a destroyed context ends in " DEAD".  A line is one write() on an
 * O_APPEND descriptor, so the lines of the addon's threads interleave whole, in time order.  Not
 * logged: lb_poll (the addon polls every 50-200 us; it is counted per ticket instead) and the
 * getters (lb_slots, lb_last_error, the table sizes, lb_same_message_mode, lb_device_count).
 *
 * Outputs are canned: verdicts 1 (written by lb_wait, as the library writes a host call's outputs
 * when it retires), a shuffling = the input reversed, found = count, every other output a fill
 * byte.  Read at lb_create / lb_create_lane (never later: the addon's threads run by then):
 *   LB_STUB_POLLS=n         lb_poll reports a ticket done on its (n+1)-th poll (default 0)
 *   LB_STUB_FAIL_LANE=append|list|balance
 *                           the lane context's lb_pubkey_table_append / lb_index_list_put /
 *                           lb_balance_table_put fails
 *   LB_STUB_FAIL_FINISH=1   lb_verify_requests_finish fails
 *   LB_STUB_UNFILLED=1      lb_sample_by_balance finds count - 1 per seed
 * No HIP, no threads of its own; a context's state is touched by the one thread that drives it. */
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "../../include/lodestar_bls.h"

#define RING 256

struct call {
  uint64_t ticket;
  uint8_t *valid, *err, *sst, *job_fast, *job_sig;
  uint32_t* job_count;
  const uint32_t* job_off;
  uint32_t n_req, n_sets, n_jobs;
  int polls;
};

struct lb_ctx {
  const char* name;
  int fd, dead, polls_needed, fail_lane, fail_finish, unfilled;
  uint32_t sm_mode, pk_size, bal_size;
  uint64_t next_ticket;
  struct call calls[RING];
  char err[96];
};

static void say(const lb_ctx* c, const char* fmt, ...) {
  char line[256];
  int n = snprintf(line, sizeof line, "%s ", c->name);
  va_list ap;
  va_start(ap, fmt);
  n += vsnprintf(line + n, sizeof line - (size_t)n - 8, fmt, ap);
  va_end(ap);
  n += snprintf(line + n, 8, "%s\n", c->dead ? " DEAD" : "");
  if (c->fd >= 0 && write(c->fd, line, (size_t)n) < 0) abort();
}

static int fail(lb_ctx* c, const char* what) {
  snprintf(c->err, sizeof c->err, "stub: %s failed", what);
  return LB_ERR_DEVICE;
}

/* first, last and a rolling hash of a word list: enough for a test to tell which list it was */
static uint32_t words_hash(uint32_t n, const uint32_t* w) {
  uint32_t h = 0;
  for (uint32_t i = 0; i < n; i++) h = h * 31u + w[i];
  return h;
}

static int make(const char* name, lb_ctx** out) {
  lb_ctx* c = calloc(1, sizeof *c);
  if (!c) return LB_ERR_OUT_OF_MEMORY;
  const char *log = getenv("LB_STUB_LOG"), *e;
  c->name = name;
  c->fd = log ? open(log, O_WRONLY | O_CREAT | O_APPEND, 0644) : -1;
  c->polls_needed = (e = getenv("LB_STUB_POLLS")) ? atoi(e) : 0;
  e = getenv("LB_STUB_FAIL_LANE");
  c->fail_lane = !e ? 0 : !strcmp(e, "append") ? 1 : !strcmp(e, "list") ? 2 : !strcmp(e, "balance") ? 3 : 0;
  c->fail_finish = (e = getenv("LB_STUB_FAIL_FINISH")) && atoi(e);
  c->unfilled = (e = getenv("LB_STUB_UNFILLED")) && atoi(e);
  c->next_ticket = 1;
  *out = c;
  say(c, "%s", name[0] == 'm' ? "lb_create" : "lb_create_lane");
  return LB_OK;
}
static int lane_fails(const lb_ctx* c, int which) { return c->name[0] == 'l' && c->fail_lane == which; }

int lb_create(int device, lb_ctx** out_ctx) { return (void)device, make("main", out_ctx); }
int lb_create_lane(int device, lb_ctx** out_ctx) { return (void)device, make("lane", out_ctx); }
int lb_mark_priority(lb_ctx* c) { return say(c, "lb_mark_priority"), LB_OK; }
int lb_destroy(lb_ctx* c) {
  if (!c) return LB_OK;
  say(c, "lb_destroy");
  c->dead = 1; /* (kept, not freed: a later call on it is logged DEAD instead of crashing) */
  return LB_OK;
}
const char* lb_last_error(const lb_ctx* c) { return c ? c->err : "stub: no error"; }
int lb_slots(const lb_ctx* c) { return (void)c, 4; }
int lb_device_count(void) { return 1; }
int lb_set_same_message_mode(lb_ctx* c, uint32_t mode) { return say(c, "lb_set_same_message_mode mode=%u", mode), c->sm_mode = mode, LB_OK; }
int lb_same_message_mode(const lb_ctx* c) { return (int)c->sm_mode; }

int lb_last_latency_clocks(const lb_ctx* c, uint64_t* out4) {
  say(c, "lb_last_latency_clocks");
  out4[0] = 100, out4[1] = 1000, out4[2] = 300, out4[3] = 5000; /* 2 us at 2000 MHz */
  return LB_OK;
}
int lb_last_stage_times(const lb_ctx* c, float* out_ms, const char** out_names, int max_stages) {
  say(c, "lb_last_stage_times");
  if (max_stages < 2) return 0;
  out_ms[0] = 0.25f, out_names[0] = "stub_a";
  out_ms[1] = 0.5f, out_names[1] = "stub_b";
  return 2;
}

/* ---- calls in flight ---- */
static struct call* submit(lb_ctx* c, const char* fn, uint32_t n_req, uint32_t n_sets, uint8_t* v, uint8_t* e,
                           uint8_t* s, uint64_t* out_ticket) {
  struct call* k = &c->calls[c->next_ticket % RING];
  memset(k, 0, sizeof *k);
  k->ticket = *out_ticket = c->next_ticket++;
  k->valid = v, k->err = e, k->sst = s, k->n_req = n_req, k->n_sets = n_sets;
  say(c, "%s n_req=%u n_sets=%u ticket=%llu", fn, n_req, n_sets, (unsigned long long)k->ticket);
  return k;
}
#define VERIFY(fn)                                                                                          \
  int fn(lb_ctx* c, const lb_request_batch* b, uint8_t* v, uint8_t* e, uint8_t* s, uint64_t* t) {            \
    return submit(c, #fn, b->n_requests, b->n_sets, v, e, s, t), LB_OK;                                      \
  }
#define VERIFY_KEYS(fn)                                                                                     \
  int fn(lb_ctx* c, const lb_request_batch* b, const lb_key_source* k, uint8_t* v, uint8_t* e, uint8_t* s,  \
         uint64_t* t) {                                                                                     \
    return (void)k, submit(c, #fn, b->n_requests, b->n_sets, v, e, s, t), LB_OK;                             \
  }
VERIFY(lb_verify_requests_async)
VERIFY(lb_verify_requests_priority_async)
VERIFY_KEYS(lb_verify_requests_keys_async)
VERIFY_KEYS(lb_verify_requests_keys_priority_async)
VERIFY_KEYS(lb_verify_requests_keys_partial_async)
int lb_verify_requests_partial_async(lb_ctx* c, const lb_request_batch* b, uint32_t flags, uint8_t* v, uint8_t* e,
                                     uint8_t* s, uint64_t* t) {
  return (void)flags, submit(c, "lb_verify_requests_partial_async", b->n_requests, b->n_sets, v, e, s, t), LB_OK;
}

int lb_verify_same_message_batch_agg_async(lb_ctx* c, const lb_same_message_batch* b, const uint8_t* agg_mask,
                                           uint8_t* out_valid, uint8_t* out_job_fast, uint8_t* out_job_sig96,
                                           uint32_t* out_job_count, uint64_t* t) {
  struct call* k = submit(c, out_job_sig96 ? "lb_verify_same_message_batch_agg_async" : "lb_verify_same_message_batch_async",
                          0, b->n_sets, NULL, NULL, out_valid, t);
  (void)agg_mask;
  k->n_jobs = b->n_jobs, k->job_off = b->job_offsets;
  k->job_fast = out_job_fast, k->job_sig = out_job_sig96, k->job_count = out_job_count;
  return LB_OK;
}
int lb_verify_same_message_batch_async(lb_ctx* c, const lb_same_message_batch* b, uint8_t* out_valid,
                                       uint8_t* out_job_fast, uint64_t* t) {
  return lb_verify_same_message_batch_agg_async(c, b, NULL, out_valid, out_job_fast, NULL, NULL, t);
}

int lb_poll(lb_ctx* c, uint64_t ticket, int32_t* out_done) {
  struct call* k = &c->calls[ticket % RING];
  *out_done = k->ticket != ticket || ++k->polls > c->polls_needed;
  if (c->dead) say(c, "lb_poll ticket=%llu", (unsigned long long)ticket);
  return LB_OK;
}
int lb_wait(lb_ctx* c, uint64_t ticket, lb_verify_stats* stats) {
  struct call* k = &c->calls[ticket % RING];
  say(c, "lb_wait ticket=%llu", (unsigned long long)ticket);
  if (k->ticket != ticket) return fail(c, "lb_wait (unknown ticket)");
  if (k->valid) memset(k->valid, 1, k->n_req), memset(k->err, 0, k->n_req);
  if (k->sst) memset(k->sst, k->valid ? 0 : 1, k->n_sets); /* (a same-message call: its per-set verdicts) */
  if (k->job_fast) memset(k->job_fast, 1, k->n_jobs);
  if (k->job_sig) memset(k->job_sig, 0xA5, (size_t)k->n_jobs * LB_SIG_COMPRESSED);
  for (uint32_t j = 0; k->job_count && j < k->n_jobs; j++) k->job_count[j] = k->job_off[j + 1] - k->job_off[j];
  if (stats) stats->batch_retries = 0, stats->batch_sigs_success = k->n_sets, stats->device_ms = 1.5;
  k->ticket = 0;
  return LB_OK;
}
int lb_partial_wait(lb_ctx* c, uint64_t ticket, uint8_t* out576) {
  say(c, "lb_partial_wait ticket=%llu", (unsigned long long)ticket);
  for (int i = 0; i < LB_GT_BYTES; i++) out576[i] = (uint8_t)i;
  return LB_OK;
}
int lb_verify_requests_finish(lb_ctx* c, uint64_t ticket, int merged_ok) {
  say(c, "lb_verify_requests_finish ticket=%llu ok=%d", (unsigned long long)ticket, merged_ok);
  return c->fail_finish ? fail(c, "lb_verify_requests_finish") : LB_OK;
}
int lb_gt_check(lb_ctx* c, uint32_t n, const uint8_t* partials576, int32_t* out_is_one) {
  return (void)partials576, say(c, "lb_gt_check n=%u", n), *out_is_one = 1, LB_OK;
}

/* ---- tables and lists ---- */
int lb_pubkey_table_append(lb_ctx* c, uint32_t n, const uint8_t* pubkeys, uint32_t pk_len, int32_t* out_bad_index) {
  (void)pubkeys, (void)out_bad_index;
  say(c, "lb_pubkey_table_append n=%u pk_len=%u", n, pk_len);
  if (lane_fails(c, 1)) return fail(c, "lb_pubkey_table_append");
  c->pk_size += n;
  return LB_OK;
}
int lb_pubkey_table_size(const lb_ctx* c, uint32_t* out_n) { return *out_n = c->pk_size, LB_OK; }
int lb_index_list_put(lb_ctx* c, uint32_t list, uint32_t n, const uint32_t* w) {
  say(c, "lb_index_list_put list=%u n=%u first=%u last=%u hash=%u", list, n, n ? w[0] : 0, n ? w[n - 1] : 0, words_hash(n, w));
  return lane_fails(c, 2) ? fail(c, "lb_index_list_put") : LB_OK;
}
int lb_index_list_shuffle(lb_ctx* c, uint32_t list, uint32_t n, const uint32_t* active, const uint8_t* seed32,
                          uint32_t* out) {
  (void)seed32;
  say(c, "lb_index_list_shuffle list=%u n=%u", list, n);
  for (uint32_t i = 0; i < n; i++) out[i] = active[n - 1 - i];
  return LB_OK;
}
int lb_balance_table_put(lb_ctx* c, uint32_t first, uint32_t n, const uint8_t* increments) {
  (void)increments;
  say(c, "lb_balance_table_put first=%u n=%u", first, n);
  if (lane_fails(c, 3)) return fail(c, "lb_balance_table_put");
  if (first + n > c->bal_size) c->bal_size = first + n;
  return LB_OK;
}
int lb_balance_table_size(const lb_ctx* c, uint32_t* out_n) { return *out_n = c->bal_size, LB_OK; }
int lb_sample_by_balance(lb_ctx* c, uint32_t n_seeds, const uint8_t* seeds32, uint32_t count, uint32_t n,
                         const uint32_t* active, uint32_t max_increment, uint32_t max_candidates, uint32_t store_list,
                         uint32_t* out_indices, uint32_t* out_found, uint32_t* out_tried) {
  (void)seeds32, (void)max_increment, (void)max_candidates;
  const uint32_t found = c->unfilled && count ? count - 1 : count;
  say(c, "lb_sample_by_balance n_seeds=%u count=%u n=%u store=%u found=%u", n_seeds, count, n, store_list, found);
  for (uint32_t s = 0; s < n_seeds; s++) {
    for (uint32_t i = 0; i < found; i++) out_indices[(size_t)s * count + i] = n ? active[(s + i) % n] : 0;
    out_found[s] = found, out_tried[s] = found + 1;
  }
  return LB_OK;
}

/* ---- one-shot operations ---- */
int lb_aggregate_pubkeys(lb_ctx* c, uint32_t n, const uint8_t* pubkeys, uint8_t* out96, uint8_t* out_status) {
  return (void)pubkeys, say(c, "lb_aggregate_pubkeys n=%u", n), memset(out96, 0x42, 96), *out_status = LB_SET_OK, LB_OK;
}
int lb_aggregate_pubkeys_indexed(lb_ctx* c, uint32_t n, const uint32_t* indices, uint8_t* out96, uint8_t* out_status) {
  return (void)indices, say(c, "lb_aggregate_pubkeys_indexed n=%u", n), memset(out96, 0x43, 96), *out_status = LB_SET_OK, LB_OK;
}
int lb_aggregate_pubkeys_list(lb_ctx* c, uint32_t list, uint32_t first, uint32_t n, uint8_t* out96, uint8_t* out_status) {
  say(c, "lb_aggregate_pubkeys_list list=%u first=%u n=%u", list, first, n);
  return memset(out96, 0x44, 96), *out_status = LB_SET_OK, LB_OK;
}
int lb_aggregate_signature_groups(lb_ctx* c, uint32_t n_groups, const uint32_t* group_offsets, const uint8_t* signatures,
                                  const uint32_t* sig_offsets, uint32_t flags, uint8_t* out96, int32_t* out_bad_index) {
  (void)group_offsets, (void)signatures, (void)sig_offsets;
  say(c, "lb_aggregate_signature_groups n_groups=%u flags=%u", n_groups, flags);
  memset(out96, 0x33, (size_t)n_groups * LB_SIG_COMPRESSED);
  for (uint32_t g = 0; g < n_groups; g++) out_bad_index[g] = -1;
  return LB_OK;
}
int lb_kzg_load_setup(lb_ctx* c, const uint8_t* g2_tau96) { return (void)g2_tau96, say(c, "lb_kzg_load_setup"), LB_OK; }
int lb_kzg_load_setup_g1(lb_ctx* c, const uint8_t* g1, int32_t* out_bad_index) {
  return (void)g1, say(c, "lb_kzg_load_setup_g1"), *out_bad_index = -1, LB_OK;
}
int lb_kzg_verify_blob_proof_batch(lb_ctx* c, uint32_t n, const uint8_t* blobs, const uint8_t* commitments48,
                                   const uint8_t* proofs48, int32_t* out_ok, uint8_t* out_status, uint8_t* out_each) {
  (void)blobs, (void)commitments48, (void)proofs48, (void)out_each;
  return say(c, "lb_kzg_verify_blob_proof_batch n=%u", n), *out_ok = 1, memset(out_status, 0, n), LB_OK;
}
int lb_kzg_blob_commitments(lb_ctx* c, uint32_t n, const uint8_t* blobs, uint8_t* out48, uint8_t* out_status) {
  (void)blobs;
  return say(c, "lb_kzg_blob_commitments n=%u", n), memset(out48, 0x51, (size_t)n * 48), memset(out_status, 0, n), LB_OK;
}
int lb_kzg_blob_proofs(lb_ctx* c, uint32_t n, const uint8_t* blobs, const uint8_t* commitments48, uint8_t* out48,
                       uint8_t* out_status) {
  (void)blobs, (void)commitments48;
  return say(c, "lb_kzg_blob_proofs n=%u", n), memset(out48, 0x52, (size_t)n * 48), memset(out_status, 0, n), LB_OK;
}
int lb_kzg_compute_proofs(lb_ctx* c, uint32_t n, const uint8_t* blobs, const uint8_t* z32, uint8_t* out48, uint8_t* out_y32,
                          uint8_t* out_status) {
  (void)blobs, (void)z32;
  say(c, "lb_kzg_compute_proofs n=%u", n);
  return memset(out48, 0x53, (size_t)n * 48), memset(out_y32, 0x54, (size_t)n * 32), memset(out_status, 0, n), LB_OK;
}
