"use strict";
// syncBalances / computeProposers / syncCommittee through the real addon on cuda:0 against what
// tests/test_js_sample.py computed with the hashlib restatement: the proposers, the committee
// (also through the priority lane, whose context mirrors the stored list) and its aggregate key.
// Run: node tests/js/gpu_sample.js DIR
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const ROOT = path.join(__dirname, "..", "..");
const V = require(path.join(ROOT, "lodestar_amd", "js", "bls_gpu_verifier.js"));
const dir = process.argv[2];
const spec = JSON.parse(fs.readFileSync(path.join(dir, "spec.json"), "utf8"));
const hex = (h) => new Uint8Array(Buffer.from(h, "hex"));
const pks = new Uint8Array(fs.readFileSync(path.join(dir, "pks.bin")));

(async () => {
  const v = new V.BlsGpuVerifier({devices: [0], seedSource: () => new Uint8Array(32)});
  try {
    const keys = [];
    for (let i = 0; i < pks.length / 96; i++) keys.push(pks.subarray(96 * i, 96 * i + 96));
    assert.strictEqual(await v.syncPubkeys(keys, 96), keys.length);
    const inc = Uint8Array.from(spec.increments);
    assert.strictEqual(await v.syncBalances(inc.subarray(0, 10)), 10);
    assert.strictEqual(await v.syncBalances(inc.subarray(5), 5), inc.length);  // overwrite and append
    await assert.rejects(v.syncBalances([1], inc.length + 1), /LB_ERR_INVALID_ARGUMENT|first beyond/);
    const active = Uint32Array.from(spec.active);
    assert.deepStrictEqual(await v.computeProposers(hex(spec.epochSeed), spec.startSlot, active), spec.proposers);
    const r = await v.syncCommittee(2, active, hex(spec.seed), spec.size);
    assert(r.indices instanceof Uint32Array);
    assert.deepStrictEqual(Array.from(r.indices), spec.committee);
    const b = v.backends[0];
    const agg = await b.aggregatePubkeys(r.indices);
    assert.deepStrictEqual(Array.from(r.aggregatePubkey), Array.from(agg));
    // the stored list serves bits sets, on the main context and on the priority lane alike
    const set = {type: "bits", list: 2, start: 0, length: spec.size, bits: hex(spec.bits), signingRoot: hex(spec.msg),
      signature: hex(spec.sig)};
    assert.strictEqual(await v.verifySignatureSets([set]), true);
    assert.strictEqual(await v.verifySignatureSets([set], {priority: true}), true);
    // a committee that cannot fill rejects and leaves the list
    await assert.rejects(v.syncCommittee(2, active, hex(spec.seed), spec.size, 32, spec.size - 1), /not filled/);
    assert.strictEqual(await v.verifySignatureSets([set]), true);
    // the raw call: an index beyond the balance table refuses
    await assert.rejects(b.sampleByBalance({seeds: hex(spec.seed), count: 1, activeIndices: Uint32Array.of(inc.length),
      maxIncrement: 32, maxCandidates: 1}), /balance table/);
    console.log("gpu sample ok");
  } finally {
    await v.close();
  }
})().catch((e) => {
  console.error(e && e.stack ? e.stack : e);
  process.exit(1);
});
