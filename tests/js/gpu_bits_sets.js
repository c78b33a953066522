"use strict";
// Index lists and sets of type "bits" through the real addon on cuda:0: syncShuffling against
// the expected shuffling, bits / index / explicit-index sets in one package (set descriptors,
// lb_verify_requests_keys_async), a flipped bit, the priority lane (whose context mirrors the
// lists) and the two-phase form.  Inputs: the directory tests/test_js_bits_sets.py wrote.
// Run: node tests/js/gpu_bits_sets.js DIR
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const ROOT = path.join(__dirname, "..", "..");
const V = require(path.join(ROOT, "lodestar_amd", "js", "bls_gpu_verifier.js"));
const dir = process.argv[2];
const spec = JSON.parse(fs.readFileSync(path.join(dir, "spec.json"), "utf8"));
const hex = (h) => new Uint8Array(Buffer.from(h, "hex"));
const pks = new Uint8Array(fs.readFileSync(path.join(dir, "pks.bin")));

function toSet(s) {
  const common = {signingRoot: hex(s.msg), signature: hex(s.sig)};
  if (s.kind === "bits") return {type: "bits", list: s.list, start: s.start, length: s.length, bits: hex(s.bits), ...common};
  if (s.kind === "single") return {type: "single", pubkey: {index: s.index}, ...common};
  return {type: "aggregate", pubkeys: s.indices.map((index) => ({index})), ...common};
}

(async () => {
  const v = new V.BlsGpuVerifier({devices: [0], seedSource: () => new Uint8Array(32)});
  try {
    const keys = [];
    for (let i = 0; i < pks.length / 96; i++) keys.push(pks.subarray(96 * i, 96 * i + 96));
    assert.strictEqual(await v.syncPubkeys(keys, 96), keys.length);
    const shuffling = await v.syncShuffling(0, Uint32Array.from(spec.active), hex(spec.seed));
    assert(shuffling instanceof Uint32Array);
    assert.deepStrictEqual(Array.from(shuffling), spec.shuffling);
    await v.putIndexList(1, Uint32Array.from(spec.sync));
    const sets = spec.sets.map(toSet);
    assert(sets.some((s) => s.type === "bits") && sets.some((s) => s.type === "single") &&
      sets.some((s) => s.type === "aggregate"));
    assert.strictEqual(await v.verifySignatureSets(sets, {batchable: true}), true);
    assert.strictEqual(await v.verifySignatureSets(sets), true);
    // the priority lane: a context of its own, its lists mirrored
    assert.strictEqual(await v.verifySignatureSets(sets, {priority: true}), true);
    assert.strictEqual(await v.verifySignatureSets(sets.slice(0, 3), {verifyOnMainThread: true}), true);
    // one participating bit cleared: other keys, false
    const k = sets.findIndex((s) => s.type === "bits");
    const wrong = sets.slice();
    const bits = Uint8Array.from(sets[k].bits);
    const j = bits.findIndex((b) => b !== 0);
    bits[j] &= bits[j] - 1;
    wrong[k] = {...sets[k], bits};
    assert.strictEqual(await v.verifySignatureSets(wrong), false);
    assert.strictEqual(await v.verifySignatureSets(wrong, {priority: true}), false);
    // an unloaded list rejects the package
    await assert.rejects(v.verifySignatureSets([{...sets[k], list: 5}]), /LB_ERR_INVALID_ARGUMENT|index list/);
    // the two-phase form through the addon
    const b = v.backends[0];
    for (const [pkg, ok] of [[sets, true], [wrong, false]]) {
      const batch = V.packRequests([pkg.slice(0, 4), pkg.slice(4)], new Uint8Array(32));
      assert(batch.setKeys instanceof Uint32Array);
      const call = await b.verifyRequestsPartial(batch);
      const merged = await b.gtCheck(call.partial);
      assert.strictEqual(merged, ok);
      const res = await b.finish(call.id, merged);
      const want = ok ? [1, 1] : [k < 4 ? 0 : 1, k < 4 ? 1 : 0];
      assert.deepStrictEqual(Array.from(res.valid), want);
    }
    console.log("gpu bits sets ok");
  } finally {
    await v.close();
  }
})().catch((e) => {
  console.error(e && e.stack ? e.stack : e);
  process.exit(1);
});
