"use strict";
// The addon's scheduling, without a GPU: the real lodestar_bls.node linked against the stand-in
// library tests/native/lb_stub.c, which logs every lb_* call (context, function, arguments) and
// answers with canned outputs.  Asserted from that log and from the resolved values: result
// shapes, priority order, mirroring into the latency lane, lane retirement, partial -> finish,
// the capacity bound and close.
//   node addon_sched.js <addon.node> <scratch dir>                (every scenario)
//   node addon_sched.js <addon.node> <scratch dir> retire <case>  (one lane-retirement case: its
//                                                                  stderr is what the parent reads)
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const {spawnSync} = require("child_process");

const [addonPath, scratch, mode, modeArg] = process.argv.slice(2);
const addon = require(path.resolve(addonPath));

const STUB_ENV = ["LB_STUB_POLLS", "LB_STUB_FAIL_LANE", "LB_STUB_FAIL_FINISH", "LB_STUB_UNFILLED", "LB_PRIO_THREAD"];
let nLogs = 0;
// A context whose library calls go to a log of its own.  The stub and the addon read their
// switches when the context is created, so they are set here, before any of its threads runs.
function open(env, opts) {
  for (const k of STUB_ENV) delete process.env[k];
  Object.assign(process.env, env || {});
  const file = path.join(scratch, `sched_${process.pid}_${nLogs++}.log`);
  process.env.LB_STUB_LOG = file;
  const ctx = new addon.Context(0, opts || {});
  const log = () =>
    fs.readFileSync(file, "utf8").split("\n").filter(Boolean).map((line) => {
      const [ctxName, fn, ...kv] = line.split(" ");
      const e = {ctx: ctxName, fn, line};
      for (const p of kv) {
        const [k, v] = p.split("=");
        if (v === undefined) e[k] = true; else e[k] = Number(v);
      }
      return e;
    });
  return {ctx, log};
}
const at = (log, pred, what) => {
  const i = log.findIndex(pred);
  assert(i >= 0, `no log line: ${what}\n${log.map((e) => e.line).join("\n")}`);
  return i;
};
const count = (log, pred) => log.filter(pred).length;
const is = (ctx, fn, more) => (e) => e.ctx === ctx && e.fn === fn && (!more || more(e));
const noDead = (log) => assert(!log.some((e) => e.DEAD), "a call on a destroyed context");
const rejects = async (p, re, code) => {
  let err = null;
  try { await p; } catch (e) { err = e; }
  assert(err, "expected a rejection");
  assert(re.test(err.message), `${err.message} !~ ${re}`);
  if (code) assert.strictEqual(err.code, code);
};

// nReq requests of one set each (one key per set); nReq also tells the calls apart in the log
function batch(nReq) {
  const off = new Uint32Array(nReq + 1), sig = new Uint32Array(nReq + 1);
  for (let i = 0; i <= nReq; i++) { off[i] = i; sig[i] = 96 * i; }
  return {requestOffsets: off, pubkeys: new Uint8Array(96 * nReq), messages: new Uint8Array(32 * nReq),
          signatures: new Uint8Array(96 * nReq), sigOffsets: sig, seed: new Uint8Array(32)};
}
function keysBatch(nReq) {
  const b = batch(nReq);
  delete b.pubkeys;
  b.setKeys = new Uint32Array(5 * nReq);  // LB_KEYS_DIRECT, validator 0
  return b;
}
const wordsHash = (w) => { let h = 0; for (const x of w) h = (Math.imul(h, 31) + x) >>> 0; return h; };
const u8 = (v, n) => v instanceof Uint8Array && v.length === n;
const VERIFY_KEYS = ["valid", "errors", "setStatus", "batchRetries", "batchSigsSuccess", "deviceMs", "workerStartNs",
                     "workerEndNs", "workerSubmittedNs", "workerRetireNs"];
// loose: a finish()'s result, or a call retired by close() -- only its start and end stamps are looked at
function checkVerdict(r, nReq, lane, loose) {
  assert.deepStrictEqual(Object.keys(r), lane ? VERIFY_KEYS.concat(["kernelMs", "kernelClockMHz", "stageMs"]) : VERIFY_KEYS);
  assert(u8(r.valid, nReq) && u8(r.errors, nReq) && u8(r.setStatus, nReq));
  assert(r.valid.every((x) => x === 1) && r.errors.every((x) => x === 0));
  assert.strictEqual(r.batchRetries, 0);
  assert.strictEqual(r.batchSigsSuccess, nReq);
  assert.strictEqual(r.deviceMs, 1.5);
  assert(r.workerStartNs > 0);
  if (!loose)
    assert(r.workerStartNs <= r.workerSubmittedNs && r.workerSubmittedNs <= r.workerRetireNs &&
           r.workerRetireNs <= r.workerEndNs);
  if (lane) {
    assert.strictEqual(r.kernelMs, 200 / 1e5);
    assert.strictEqual(r.kernelClockMHz, 2000);
    assert.deepStrictEqual(r.stageMs, {stub_a: 0.25, stub_b: 0.5});
  }
}

// ---- 1. result shapes: every method of Context (the list in the addon's Init) ----------------
async function shapes() {
  const {ctx, log} = open();
  assert.deepStrictEqual(Object.getOwnPropertyNames(addon.Context.prototype).filter((m) => m !== "constructor").sort(), [
    "aggregatePubkeys", "aggregateSignatureGroups", "balanceTablePut", "close", "finish", "gtCheck", "indexListPut",
    "indexListShuffle", "kzgBlobCommitments", "kzgBlobProofs", "kzgComputeProofs", "kzgLoadSetup", "kzgLoadSetupG1",
    "kzgVerifyBlobProofBatch", "sampleByBalance", "syncPubkeys", "verifyRequests", "verifyRequestsPartial",
    "verifySameMessage"]);
  assert.strictEqual(ctx.device, 0);
  assert.strictEqual(ctx.capacity, 4);
  assert.strictEqual(ctx.sameMessageRandomized, false);

  checkVerdict(await ctx.verifyRequests(batch(3)), 3, false);
  checkVerdict(await ctx.verifyRequests(batch(0)), 0, false);
  const p = await ctx.verifyRequestsPartial(batch(2));
  assert.deepStrictEqual(Object.keys(p), ["id", "partial"]);
  assert(typeof p.id === "number" && u8(p.partial, 576) && p.partial[575] === (575 & 255));
  checkVerdict(await ctx.finish(p.id, true), 2, false, true);
  assert.strictEqual(await ctx.gtCheck(new Uint8Array(2 * 576)), true);

  const sm = {jobOffsets: new Uint32Array([0, 2, 3]), pubkeys: new Uint8Array(3 * 96), signatures: new Uint8Array(3 * 96),
              sigOffsets: new Uint32Array([0, 96, 192, 288]), messages: new Uint8Array(2 * 32), seed: new Uint8Array(32)};
  const SM_KEYS = ["valid", "jobFast", "retriedJobs", "fastSets", "deviceMs", "workerStartNs", "workerEndNs"];
  let r = await ctx.verifySameMessage(sm);
  assert.deepStrictEqual(Object.keys(r), SM_KEYS);
  assert(u8(r.valid, 3) && u8(r.jobFast, 2) && r.valid[2] === 1 && r.jobFast[1] === 1);
  assert(r.retriedJobs === 0 && r.fastSets === 3 && r.deviceMs === 1.5 && r.workerStartNs <= r.workerEndNs);
  r = await ctx.verifySameMessage(sm, {aggregate: true, mask: new Uint8Array(3)});
  assert.deepStrictEqual(Object.keys(r), SM_KEYS.concat(["jobSignatures", "jobCounts"]));
  assert(u8(r.jobSignatures, 2 * 96) && r.jobSignatures[191] === 0xa5);
  assert(r.jobCounts instanceof Uint32Array);
  assert.deepStrictEqual(Array.from(r.jobCounts), [2, 1]);

  r = await ctx.aggregateSignatureGroups({groupOffsets: new Uint32Array([0, 2, 3]), signatures: new Uint8Array(3 * 96),
                                          sigOffsets: new Uint32Array([0, 96, 192, 288])}, {noCheck: true});
  assert.deepStrictEqual(Object.keys(r), ["signatures", "badIndex"]);
  assert(u8(r.signatures, 2 * 96) && r.signatures[0] === 0x33 && r.badIndex instanceof Int32Array);
  assert.deepStrictEqual(Array.from(r.badIndex), [-1, -1]);

  assert.strictEqual(await ctx.syncPubkeys(new Uint8Array(5 * 48), 48), 5);
  assert.strictEqual(await ctx.syncPubkeys(new Uint8Array(2 * 96), 96), 7);
  r = await ctx.aggregatePubkeys(new Uint8Array(2 * 96));
  assert(u8(r, 96) && r[0] === 0x42);
  r = await ctx.aggregatePubkeys(new Uint32Array([1, 2, 3]));
  assert(u8(r, 96) && r[0] === 0x43);
  assert.strictEqual(await ctx.indexListPut(1, new Uint32Array([4, 5, 6])), 3);
  r = await ctx.indexListShuffle(2, new Uint32Array([4, 5, 6, 7]), new Uint8Array(32));
  assert(r instanceof Uint32Array);
  assert.deepStrictEqual(Array.from(r), [7, 6, 5, 4]);
  assert.strictEqual(await ctx.balanceTablePut(0, new Uint8Array(9)), 9);
  r = await ctx.sampleByBalance({seeds: new Uint8Array(64), count: 3, activeIndices: new Uint32Array([10, 11, 12, 13]),
                                 maxIncrement: 32, maxCandidates: 100});
  assert.deepStrictEqual(Object.keys(r), ["indices", "found", "tried"]);
  assert(r.indices instanceof Uint32Array && r.found instanceof Uint32Array && r.tried instanceof Uint32Array);
  assert.deepStrictEqual(Array.from(r.indices), [10, 11, 12, 11, 12, 13]);
  assert.deepStrictEqual([Array.from(r.found), Array.from(r.tried)], [[3, 3], [4, 4]]);

  assert.strictEqual(await ctx.kzgLoadSetup(new Uint8Array(96)), undefined);
  assert.strictEqual(await ctx.kzgLoadSetupG1(new Uint8Array(4096 * 48)), undefined);
  const blobs = new Uint8Array(2 * 131072);
  r = await ctx.kzgVerifyBlobProofBatch(blobs, new Uint8Array(96), new Uint8Array(96));
  assert.deepStrictEqual(Object.keys(r), ["ok", "status"]);
  assert(r.ok === true && u8(r.status, 2));
  r = await ctx.kzgBlobCommitments(blobs);
  assert.deepStrictEqual(Object.keys(r), ["commitments", "status"]);
  assert(u8(r.commitments, 96) && r.commitments[95] === 0x51 && u8(r.status, 2));
  r = await ctx.kzgBlobProofs(blobs, new Uint8Array(96));
  assert.deepStrictEqual(Object.keys(r), ["proofs", "status"]);
  assert(u8(r.proofs, 96) && r.proofs[95] === 0x52 && u8(r.status, 2));
  r = await ctx.kzgComputeProofs(blobs, new Uint8Array(64));
  assert.deepStrictEqual(Object.keys(r), ["proofs", "ys", "status"]);
  assert(u8(r.proofs, 96) && r.proofs[0] === 0x53 && u8(r.ys, 64) && r.ys[63] === 0x54 && u8(r.status, 2));
  r = await ctx.kzgBlobCommitments(new Uint8Array(0));
  assert(u8(r.commitments, 0) && u8(r.status, 0));

  // bad arguments reject with a TypeError and never reach the library
  const before = log().length;
  await rejects(ctx.verifyRequests({}), /missing requestOffsets/);
  await rejects(ctx.verifyRequests(), /verifyRequests\(batch/);
  await rejects(ctx.gtCheck(new Uint8Array(5)), /576 bytes each/);
  await rejects(ctx.syncPubkeys(new Uint8Array(96), 50), /pkLen must be 48 or 96/);
  await rejects(ctx.aggregatePubkeys(new Uint8Array(0)), /EMPTY_AGGREGATE_ARRAY/);
  await rejects(ctx.kzgBlobProofs(blobs, new Uint8Array(95)), /commitments: 48 bytes per blob/);
  await rejects(ctx.verifySameMessage({...sm, pubkeys: undefined, pubkeyIndices: new Uint32Array([1, 0x80000002, 3])}),
                /pubkeyIndices name pubkey rows/);
  await rejects(ctx.verifyRequests({...batch(1), pubkeys: undefined, pubkeyIndices: new Uint32Array([0x80000000])}),
                /pubkeyIndices name pubkey rows/);
  await rejects(ctx.finish("x", true), /finish\(id: number, mergedOk: boolean\)/);
  assert.strictEqual(log().length, before);
  assert.strictEqual(await ctx.close(), undefined);
  noDead(log());

  // sameMessageRandomized: the mode is set on both contexts before any call
  const o = open({}, {sameMessageRandomized: true, capacity: 3});
  assert(o.ctx.sameMessageRandomized === true && o.ctx.capacity === 3);
  await o.ctx.close();
  const l = o.log();
  at(l, is("main", "lb_set_same_message_mode", (e) => e.mode === 1), "main mode");
  at(l, is("lane", "lb_set_same_message_mode", (e) => e.mode === 1), "lane mode");
}

// ---- 2. priority calls ---------------------------------------------------------------------------
async function priority() {
  // with the lane: marked on the main context, run on the lane's
  let {ctx, log} = open();
  checkVerdict(await ctx.verifyRequests(batch(2), {priority: true}), 2, true);
  checkVerdict(await ctx.verifyRequests(keysBatch(3), {priority: true}), 3, true);
  await ctx.verifyRequests(keysBatch(4));
  await ctx.finish((await ctx.verifyRequestsPartial(keysBatch(5))).id, false);
  await ctx.verifyRequests(batch(6), {priority: false});
  await ctx.close();
  let l = log();
  noDead(l);
  const mark = at(l, is("main", "lb_mark_priority"), "mark");
  const run = at(l, is("lane", "lb_verify_requests_priority_async", (e) => e.n_req === 2), "lane priority call");
  assert(mark < run);
  assert.strictEqual(count(l, is("main", "lb_mark_priority")), 2);
  at(l, is("lane", "lb_verify_requests_keys_priority_async", (e) => e.n_req === 3), "lane keys priority call");
  at(l, is("main", "lb_verify_requests_keys_async", (e) => e.n_req === 4), "keys call");
  at(l, is("main", "lb_verify_requests_keys_partial_async", (e) => e.n_req === 5), "keys partial call");
  at(l, is("main", "lb_verify_requests_finish", (e) => e.ok === 0), "finish(false)");
  at(l, is("main", "lb_verify_requests_async", (e) => e.n_req === 6), "priority: false");
  assert.strictEqual(count(l, (e) => e.ctx === "main" && /priority_async/.test(e.fn)), 0);
  assert.strictEqual(count(l, (e) => e.ctx === "lane" && e.fn === "lb_wait"), 2);

  // without it (LB_PRIO_THREAD=0): on the main context, ahead of the queued non-priority tasks
  // and behind earlier priority ones.  One slot and slow polls keep calls 2 and 3 queued while
  // the priority calls 11 and 12 arrive (all five are queued in this one synchronous stretch).
  ({ctx, log} = open({LB_PRIO_THREAD: "0", LB_STUB_POLLS: "40"}, {capacity: 1}));
  const ps = [ctx.verifyRequests(batch(1)), ctx.verifyRequests(batch(2)), ctx.syncPubkeys(new Uint8Array(96), 96),
              ctx.verifyRequests(batch(3)), ctx.verifyRequests(batch(11), {priority: true}),
              ctx.verifyRequests(keysBatch(12), {priority: true})];
  const rs = await Promise.all(ps);
  checkVerdict(rs[4], 11, false);
  checkVerdict(rs[5], 12, false);
  await ctx.close();
  l = log();
  noDead(l);
  assert.strictEqual(count(l, (e) => e.ctx === "lane"), 0);
  assert.strictEqual(count(l, is("main", "lb_mark_priority")), 0);
  const p11 = at(l, is("main", "lb_verify_requests_priority_async", (e) => e.n_req === 11), "priority 11");
  const p12 = at(l, is("main", "lb_verify_requests_keys_priority_async", (e) => e.n_req === 12), "priority 12");
  const n1 = at(l, is("main", "lb_verify_requests_async", (e) => e.n_req === 1), "call 1");
  const n2 = at(l, is("main", "lb_verify_requests_async", (e) => e.n_req === 2), "call 2");
  const sync = at(l, is("main", "lb_pubkey_table_append"), "append");
  const n3 = at(l, is("main", "lb_verify_requests_async", (e) => e.n_req === 3), "call 3");
  assert(p11 < p12 && p12 < n2 && n1 < n2 && n2 < sync && sync < n3, l.map((e) => e.line).join("\n"));
  for (const t of [1, 2, 3, 4, 5])
    assert.strictEqual(count(l, is("main", "lb_wait", (e) => e.ticket === t)), 1, `ticket ${t} waited once`);
}

// ---- 3. mirroring into the lane --------------------------------------------------------------
async function mirroring() {
  let {ctx, log} = open();
  const order = (l, fn, more) => {
    const m = at(l, is("main", fn, more), "main " + fn), n = at(l, is("lane", fn, more), "lane " + fn);
    assert(m < n, `${fn}: main first`);
    return l[n];
  };
  // (the lane's line is in the log when the promise resolves: the task resolves after the lane)
  assert.strictEqual(await ctx.syncPubkeys(new Uint8Array(3 * 48), 48), 3);
  let e = order(log(), "lb_pubkey_table_append");
  assert(e.n === 3 && e.pk_len === 48);

  const idx = new Uint32Array([9, 8, 7, 6, 5]);
  assert.strictEqual(await ctx.indexListPut(2, idx), 5);
  e = order(log(), "lb_index_list_put", (x) => x.list === 2);
  assert(e.n === 5 && e.first === 9 && e.last === 5 && e.hash === wordsHash(idx));

  const active = new Uint32Array([1, 2, 3, 4, 5, 6]);
  const sh = await ctx.indexListShuffle(3, active, new Uint8Array(32));
  let l = log();
  at(l, is("main", "lb_index_list_shuffle", (x) => x.list === 3 && x.n === 6), "shuffle");
  assert.strictEqual(count(l, is("lane", "lb_index_list_shuffle")), 0);
  e = l[at(l, is("lane", "lb_index_list_put", (x) => x.list === 3), "the lane's put of the shuffling")];
  assert(e.n === 6 && e.first === 6 && e.last === 1 && e.hash === wordsHash(sh));  // the computed shuffling

  assert.strictEqual(await ctx.balanceTablePut(4, new Uint8Array(6)), 10);
  e = order(log(), "lb_balance_table_put");
  assert(e.first === 4 && e.n === 6);
  assert.strictEqual(await ctx.balanceTablePut(0, new Uint8Array(2)), 10);
  assert.strictEqual(count(log(), is("lane", "lb_balance_table_put", (x) => x.first === 0 && x.n === 2)), 1);

  const q = {seeds: new Uint8Array(32), count: 4, activeIndices: new Uint32Array([20, 21, 22, 23, 24]), maxIncrement: 32,
             maxCandidates: 64};
  let r = await ctx.sampleByBalance({...q, storeList: 5});
  assert.deepStrictEqual(Object.keys(r), ["indices", "found", "tried"]);
  l = log();
  at(l, is("main", "lb_sample_by_balance", (x) => x.store === 5 && x.count === 4 && x.n === 5), "sample");
  e = l[at(l, is("lane", "lb_index_list_put", (x) => x.list === 5), "the lane's put of the committee")];
  assert(e.n === 4 && e.first === 20 && e.last === 23 && e.hash === wordsHash(r.indices));
  assert.strictEqual(count(l, is("main", "lb_aggregate_pubkeys_list")), 0);

  r = await ctx.sampleByBalance({...q, storeList: 6, aggregate: true});
  assert.deepStrictEqual(Object.keys(r), ["indices", "found", "tried", "aggregatePubkey"]);
  assert(u8(r.aggregatePubkey, 96) && r.aggregatePubkey[0] === 0x44);
  l = log();
  e = l[at(l, is("main", "lb_aggregate_pubkeys_list"), "aggregate of the stored list")];
  assert(e.list === 6 && e.first === 0 && e.n === 4);
  at(l, is("lane", "lb_index_list_put", (x) => x.list === 6), "the lane's put of list 6");

  // no storeList (aggregate or not), or two seeds: nothing for the lane
  let before = count(log(), (x) => x.ctx === "lane");
  r = await ctx.sampleByBalance({...q, aggregate: true});
  assert.deepStrictEqual(Object.keys(r), ["indices", "found", "tried"]);
  await ctx.sampleByBalance({...q, storeList: null});
  await ctx.sampleByBalance({...q, seeds: new Uint8Array(64), storeList: 7});
  assert.strictEqual(count(log(), (x) => x.ctx === "lane"), before);
  assert.strictEqual(count(log(), is("main", "lb_aggregate_pubkeys_list")), 1);
  await ctx.close();
  noDead(log());

  // a sample left unfilled: no lane call, no aggregate
  ({ctx, log} = open({LB_STUB_UNFILLED: "1"}));
  r = await ctx.sampleByBalance({...q, storeList: 5, aggregate: true});
  assert.deepStrictEqual(Object.keys(r), ["indices", "found", "tried"]);
  assert.deepStrictEqual(Array.from(r.found), [3]);
  assert.strictEqual(r.indices[3], 0xffffffff);  // LB_SAMPLE_NONE
  await ctx.close();
  l = log();
  assert.strictEqual(count(l, is("lane", "lb_index_list_put")), 0);
  assert.strictEqual(count(l, is("main", "lb_aggregate_pubkeys_list")), 0);

  // without a lane (LB_PRIO_THREAD=0) the same calls resolve from the main context alone
  ({ctx, log} = open({LB_PRIO_THREAD: "0"}));
  assert.strictEqual(await ctx.syncPubkeys(new Uint8Array(96), 96), 1);
  assert.strictEqual(await ctx.indexListPut(0, idx), 5);
  assert.strictEqual(await ctx.balanceTablePut(1, new Uint8Array(1)), 2);
  await ctx.sampleByBalance({...q, storeList: 5});
  await ctx.close();
  assert.strictEqual(count(log(), (x) => x.ctx === "lane"), 0);
}

// ---- 4. lane retirement (one case per process: the sentence on stderr is the parent's to read) --
const RETIRE = {
  append: {fail: "append", what: "pubkey table", run: async (ctx) => assert.strictEqual(await ctx.syncPubkeys(new Uint8Array(96), 96), 1)},
  list: {fail: "list", what: "index lists", run: async (ctx) => assert.strictEqual(await ctx.indexListPut(1, new Uint32Array([3, 4])), 2)},
  shuffle: {fail: "list", what: "index lists", run: async (ctx) =>
    assert.deepStrictEqual(Array.from(await ctx.indexListShuffle(1, new Uint32Array([3, 4]), new Uint8Array(32))), [4, 3])},
  sample: {fail: "list", what: "index lists", run: async (ctx) => {
    const r = await ctx.sampleByBalance({seeds: new Uint8Array(32), count: 2, activeIndices: new Uint32Array([7, 8, 9]),
                                         maxIncrement: 32, maxCandidates: 64, storeList: 1});
    assert.deepStrictEqual(Array.from(r.indices), [7, 8]);
  }},
  balance: {fail: "balance", what: "balance table", run: async (ctx) => assert.strictEqual(await ctx.balanceTablePut(2, new Uint8Array(3)), 5)},
};
async function retireChild(name) {
  const {ctx, log} = open({LB_STUB_FAIL_LANE: RETIRE[name].fail});
  checkVerdict(await ctx.verifyRequests(batch(1), {priority: true}), 1, true);  // the lane works ...
  await RETIRE[name].run(ctx);                                                  // ... fails to follow: the task still resolves
  checkVerdict(await ctx.verifyRequests(batch(2), {priority: true}), 2, false);
  checkVerdict(await ctx.verifyRequests(keysBatch(3), {priority: true}), 3, false);
  // later mirrored operations resolve from the main context alone
  assert.strictEqual(await ctx.indexListPut(4, new Uint32Array([1])), 1);
  await ctx.close();
  const l = log();
  noDead(l);
  at(l, is("lane", "lb_verify_requests_priority_async", (e) => e.n_req === 1), "before: on the lane");
  at(l, is("main", "lb_verify_requests_priority_async", (e) => e.n_req === 2), "after: on the main context");
  at(l, is("main", "lb_verify_requests_keys_priority_async", (e) => e.n_req === 3), "after: keys, on the main context");
  assert.strictEqual(count(l, (e) => e.ctx === "lane" && /_async$/.test(e.fn)), 1);
  assert.strictEqual(count(l, is("lane", "lb_index_list_put", (e) => e.list === 4)), 0);
  assert(at(l, is("lane", "lb_destroy"), "lane destroyed") < at(l, is("main", "lb_destroy"), "main destroyed"));
}
function retirement() {
  for (const name of Object.keys(RETIRE)) {
    const r = spawnSync(process.execPath, [__filename, addonPath, scratch, "retire", name], {encoding: "utf8"});
    assert.strictEqual(r.status, 0, `${name}: ${r.stdout}${r.stderr}`);
    const sentence = `lodestar_bls: latency lane retired (its ${RETIRE[name].what} could not follow: stub: ` +
                     `${{append: "lb_pubkey_table_append", list: "lb_index_list_put", balance: "lb_balance_table_put"}[RETIRE[name].fail]}` +
                     ` failed); priority calls run on the main context\n`;
    assert.strictEqual(r.stderr, sentence, name);
  }
}

// ---- 5. two-phase --------------------------------------------------------------------------------
async function twoPhase() {
  let {ctx, log} = open();
  const a = await ctx.verifyRequestsPartial(batch(3));
  const b = await ctx.verifyRequestsPartial(batch(4));
  assert(a.id !== b.id && u8(a.partial, 576));
  const afterPartials = Number(process.hrtime.bigint());  // (the clock of workerStartNs)
  await rejects(ctx.finish(a.id + b.id + 1, true), /unknown or already finished two-phase call/, "LB_ERR_INVALID_ARGUMENT");
  const rb = await ctx.finish(b.id, false);  // out of order
  const ra = await ctx.finish(a.id, true);
  checkVerdict(ra, 3, false, true);
  checkVerdict(rb, 4, false, true);
  assert(ra.workerEndNs > afterPartials && rb.workerEndNs > afterPartials);
  assert(ra.workerStartNs < afterPartials && rb.workerStartNs < afterPartials, "workerStartNs is the call's, not the finish's");
  assert(ra.workerStartNs < rb.workerStartNs);
  await rejects(ctx.finish(a.id, true), /unknown or already finished two-phase call/, "LB_ERR_INVALID_ARGUMENT");
  await ctx.close();
  let l = log();
  noDead(l);
  const ta = l[at(l, is("main", "lb_verify_requests_partial_async", (e) => e.n_req === 3), "partial a")].ticket;
  const tb = l[at(l, is("main", "lb_verify_requests_partial_async", (e) => e.n_req === 4), "partial b")].ticket;
  for (const [t, ok] of [[ta, 1], [tb, 0]]) {
    const pw = at(l, is("main", "lb_partial_wait", (e) => e.ticket === t), "partial_wait");
    const fi = at(l, is("main", "lb_verify_requests_finish", (e) => e.ticket === t && e.ok === ok), "finish");
    const w = at(l, is("main", "lb_wait", (e) => e.ticket === t), "wait");
    assert(pw < fi && fi < w);
    assert.strictEqual(count(l, is("main", "lb_wait", (e) => e.ticket === t)), 1);
    assert.strictEqual(count(l, is("main", "lb_verify_requests_finish", (e) => e.ticket === t)), 1);
  }

  // a failing lb_verify_requests_finish rejects, and the call is still waited on once
  ({ctx, log} = open({LB_STUB_FAIL_FINISH: "1"}));
  const c = await ctx.verifyRequestsPartial(batch(2));
  await rejects(ctx.finish(c.id, true), /stub: lb_verify_requests_finish failed/, "LB_ERR_DEVICE");
  await rejects(ctx.finish(c.id, true), /unknown or already finished/);
  checkVerdict(await ctx.verifyRequests(batch(1)), 1, false);  // the context goes on
  await ctx.close();
  l = log();
  noDead(l);
  const tc = l[at(l, is("main", "lb_verify_requests_partial_async"), "partial c")].ticket;
  assert.strictEqual(count(l, is("main", "lb_wait", (e) => e.ticket === tc)), 1);
  assert.strictEqual(count(l, is("main", "lb_verify_requests_finish")), 1);
}

// ---- 6. capacity ---------------------------------------------------------------------------------
async function capacity() {
  const {ctx, log} = open({LB_STUB_POLLS: "40"}, {capacity: 2});
  assert.strictEqual(ctx.capacity, 2);
  const sm = {jobOffsets: new Uint32Array([0, 1]), pubkeys: new Uint8Array(96), signatures: new Uint8Array(96),
              sigOffsets: new Uint32Array([0, 96]), messages: new Uint8Array(32), seed: new Uint8Array(32)};
  const ps = [];
  for (let i = 1; i <= 6; i++) ps.push(i === 4 ? ctx.verifySameMessage(sm) : ctx.verifyRequests(batch(i)));
  ps.push(ctx.verifyRequests(batch(9), {priority: true}));  // (the lane's: beside the two)
  const rs = await Promise.all(ps);
  rs.forEach((r, i) => i !== 3 && checkVerdict(r, i === 6 ? 9 : i + 1, i === 6));
  await ctx.close();
  const l = log().filter((e) => e.ctx === "main");
  let inFlight = 0, most = 0;
  const seen = new Set();
  for (const e of l) {
    if (/_async$/.test(e.fn)) { inFlight++; seen.add(e.ticket); }
    if (e.fn === "lb_wait") { inFlight--; assert(seen.delete(e.ticket), "waited once, after its submit"); }
    assert(inFlight <= 2, "more than `capacity` calls in flight");
    most = Math.max(most, inFlight);
  }
  assert.strictEqual(most, 2);  // (and the slots are used: calls overlap)
  assert.strictEqual(seen.size, 0);
  assert.strictEqual(count(l, (e) => /_async$/.test(e.fn)), 6);
  // in submission order, retired oldest first
  assert.deepStrictEqual(l.filter((e) => e.fn === "lb_wait").map((e) => e.ticket), [1, 2, 3, 4, 5, 6]);
}

// ---- 7. close --------------------------------------------------------------------------------------
async function closing() {
  // no poll ever reports a call done, and close() is startable beside the three in flight: it is
  // close() that waits for them
  const {ctx, log} = open({LB_STUB_POLLS: "100000000"}, {capacity: 4});
  const unfinished = await ctx.verifyRequestsPartial(batch(7));
  const part = await ctx.verifyRequestsPartial(batch(8));
  const ps = [ctx.verifyRequests(batch(1)), ctx.verifyRequests(batch(2)), ctx.finish(part.id, true),
              ctx.syncPubkeys(new Uint8Array(96), 96),
              ctx.verifyRequests(batch(4), {priority: true}), ctx.verifyRequests(batch(5), {priority: true})];
  const closed = ctx.close();
  const late = ctx.verifyRequests(batch(6));
  const again = ctx.close();
  await rejects(late, /QUEUE_ERROR_QUEUE_ABORTED: context closed/, "LB_ERR_INVALID_ARGUMENT");
  assert.strictEqual(await again, undefined);
  const rs = await Promise.all(ps);
  [1, 2, 8].forEach((n, i) => checkVerdict(rs[i], n, false, true));
  assert.strictEqual(rs[3], 1);
  checkVerdict(rs[4], 4, true);
  checkVerdict(rs[5], 5, true);
  assert.strictEqual(await closed, undefined);
  await rejects(ctx.syncPubkeys(new Uint8Array(96), 96), /QUEUE_ERROR_QUEUE_ABORTED/);
  await rejects(ctx.finish(unfinished.id, true), /QUEUE_ERROR_QUEUE_ABORTED/);
  assert.strictEqual(await ctx.close(), undefined);
  const l = log();
  noDead(l);
  const dl = at(l, is("lane", "lb_destroy"), "lane destroyed"), dm = at(l, is("main", "lb_destroy"), "main destroyed");
  assert(dl < dm && dm === l.length - 1, "lane first, the main context last");
  assert.strictEqual(count(l, (e) => e.fn === "lb_destroy"), 2);
  for (const c of ["main", "lane"]) {
    const sub = l.filter((e) => e.ctx === c && /_async$/.test(e.fn));
    assert.strictEqual(sub.length, c === "main" ? 4 : 2);
    for (const s of sub) {
      const n = count(l, is(c, "lb_wait", (e) => e.ticket === s.ticket));
      // (a two-phase call never finished is dropped with the context, as the library allows)
      assert.strictEqual(n, s.n_req === 7 ? 0 : 1, `${c} ticket ${s.ticket} waited ${n} times`);
    }
  }
  at(l, is("lane", "lb_pubkey_table_append"), "the lane's queue drained");
}

async function main() {
  if (mode === "retire") return retireChild(modeArg);
  const all = {shapes, priority, mirroring, retirement, twoPhase, capacity, closing};
  for (const name of Object.keys(all)) {
    await all[name]();
    console.log("ok", name);
  }
  console.log("addon sched ok");
}
main().catch((e) => {
  console.error(e && e.stack || e);
  process.exit(1);
});
