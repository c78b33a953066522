"use strict";
// verifyAndAggregateSameMessage / aggregateSignatureGroups through BlsGpuVerifier and
// BlsGpuSingleThreadVerifier with a stand-in addon (no GPU): the aggregate flag and the mask
// reach the context, the result is shaped {valid, signature, count}, and a call without the
// option reaches the context exactly as before.
const assert = require("assert");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "bls_gpu_verifier.js"));

const calls = [];
class MockContext {
  constructor(device, opts) {
    this.capacity = (opts && opts.capacity) || 2;
  }
  // a set is invalid when its signature starts with 0xff; a job's "aggregate" is a tag:
  // byte 0 = how many were summed, then their positions in the job
  async verifySameMessage(...args) {
    calls.push(args);
    const [b, o] = args;
    const nJobs = b.jobOffsets.length - 1;
    const nSets = b.jobOffsets[nJobs];
    const valid = new Uint8Array(nSets);
    for (let i = 0; i < nSets; i++) valid[i] = b.signatures[b.sigOffsets[i]] === 0xff ? 0 : 1;
    const jobFast = new Uint8Array(nJobs);
    const r = {valid, jobFast, retriedJobs: 0, fastSets: 0, deviceMs: 0};
    if (o && o.aggregate) {
      r.jobSignatures = new Uint8Array(96 * nJobs);
      r.jobCounts = new Uint32Array(nJobs);
    }
    for (let j = 0; j < nJobs; j++) {
      let all = 1;
      for (let i = b.jobOffsets[j]; i < b.jobOffsets[j + 1]; i++) {
        if (!valid[i]) all = 0;
        if (r.jobCounts && valid[i] && (!o.mask || o.mask[i])) {
          r.jobSignatures[96 * j + 1 + r.jobCounts[j]] = i - b.jobOffsets[j];
          r.jobCounts[j]++;
        }
      }
      jobFast[j] = all;
      if (r.jobCounts) r.jobSignatures[96 * j] = r.jobCounts[j];
    }
    return r;
  }
  async aggregateSignatureGroups(b, o) {
    calls.push([b, o]);
    const n = b.groupOffsets.length - 1;
    const badIndex = new Int32Array(n).fill(-1);
    for (let g = 0; g < n; g++)
      for (let i = b.groupOffsets[g]; i < b.groupOffsets[g + 1]; i++)
        if (b.signatures[b.sigOffsets[i]] === 0xff && badIndex[g] < 0) badIndex[g] = i;
    const signatures = new Uint8Array(96 * n);
    for (let g = 0; g < n; g++) signatures[96 * g] = b.groupOffsets[g + 1] - b.groupOffsets[g];
    return {signatures, badIndex};
  }
  async close() {}
}
const addon = {Context: MockContext};
const mkSets = (n, bad = []) =>
  Array.from({length: n}, (_, i) => ({publicKey: new Uint8Array(96), signature: new Uint8Array(96).fill(bad.includes(i) ? 0xff : 1)}));

async function main() {
  let failed = 0;
  const check = async (name, fn) => {
    try {
      await fn();
      console.log("ok", name);
    } catch (e) {
      failed++;
      console.log("FAILED", name, e && e.stack);
    }
  };
  const root = new Uint8Array(32);

  await check("pool: flag and mask go down, {valid, signature, count} comes up", async () => {
    calls.length = 0;
    const v = new V.BlsGpuVerifier({addon});
    const include = Array.from({length: 200}, (_, i) => i !== 5);
    // 200 sets stay one job; a plain job and an all-invalid job share the device call
    const [big, plain, none] = await Promise.all([
      v.verifyAndAggregateSameMessage(mkSets(200, [3]), root, {include}),
      v.verifySignatureSetsSameMessage(mkSets(2), root),
      v.verifyAndAggregateSameMessage(mkSets(2, [0, 1]), root),
    ]);
    assert.strictEqual(calls.length, 1);
    const [batch, opts] = calls[0];
    assert.deepStrictEqual(Array.from(batch.jobOffsets), [0, 200, 202, 204]);
    assert.strictEqual(opts.aggregate, true);
    assert.ok(opts.mask instanceof Uint8Array && opts.mask.length === 204);
    assert.deepStrictEqual(Array.from(opts.mask), Array.from({length: 204}, (_, i) => (i === 5 ? 0 : 1)));
    assert.deepStrictEqual(big.valid, Array.from({length: 200}, (_, i) => i !== 3));
    assert.strictEqual(big.count, 198);
    assert.ok(big.signature instanceof Uint8Array && big.signature.length === 96);
    assert.deepStrictEqual(Array.from(big.signature.subarray(0, 6)), [198, 0, 1, 2, 4, 6]);
    assert.deepStrictEqual(plain, [true, true]);
    assert.deepStrictEqual(none, {valid: [false, false], signature: null, count: 0});
    await v.close();
  });
  await check("pool: a call without the option is unchanged", async () => {
    calls.length = 0;
    const v = new V.BlsGpuVerifier({addon});
    assert.deepStrictEqual(await v.verifySignatureSetsSameMessage(mkSets(3, [1]), root), [true, false, true]);
    assert.strictEqual(calls.length, 1);
    assert.strictEqual(calls[0].length, 1); // verifySameMessage(batch), no second argument
    await v.close();
  });
  await check("single thread", async () => {
    calls.length = 0;
    const v = new V.BlsGpuSingleThreadVerifier({addon});
    const r = await v.verifyAndAggregateSameMessage(mkSets(4, [2]), root, {include: [true, false, true, true]});
    assert.deepStrictEqual(Array.from(calls[0][1].mask), [1, 0, 1, 1]);
    assert.strictEqual(calls[0][1].aggregate, true);
    assert.deepStrictEqual(r.valid, [true, true, false, true]);
    assert.strictEqual(r.count, 2);
    assert.deepStrictEqual(Array.from(r.signature.subarray(0, 3)), [2, 0, 3]);
    assert.deepStrictEqual(await v.verifySignatureSetsSameMessage(mkSets(2), root), [true, true]);
    assert.strictEqual(calls[1].length, 1);
    await assert.rejects(v.verifyAndAggregateSameMessage(mkSets(2), root, {include: [true]}), /include/);
    await v.close();
  });
  await check("aggregateSignatureGroups packs groups and throws on a bad one", async () => {
    calls.length = 0;
    const v = new V.BlsGpuVerifier({addon});
    const sig = (b) => new Uint8Array(96).fill(b);
    const out = await v.aggregateSignatureGroups([[sig(1), sig(2)], [sig(3)]], {noCheck: true});
    assert.deepStrictEqual(Array.from(calls[0][0].groupOffsets), [0, 2, 3]);
    assert.deepStrictEqual(Array.from(calls[0][0].sigOffsets), [0, 96, 192, 288]);
    assert.deepStrictEqual(calls[0][1], {noCheck: true});
    assert.deepStrictEqual(out.map((s) => [s.length, s[0]]), [[96, 2], [96, 1]]);
    await assert.rejects(v.aggregateSignatureGroups([[sig(1)], [sig(2), sig(0xff)]]), /invalid signature 2 \(group 1\)/);
    await assert.rejects(v.aggregateSignatureGroups([[sig(1)], []]), /EMPTY_AGGREGATE_ARRAY/);
    await v.close();
  });
  console.log(`${failed} failed`);
  process.exit(failed ? 1 : 0);
}
main();
