"use strict";
// Sets of type "bits" on the JS host with a mock backend (no GPU): a package whose keys are all
// validator indices or bits sets reaches the addon as set descriptors (setKeys / keyPool /
// keyBits); one that holds a key travelling by its bytes falls back to today's form, its bits
// sets expanded from the host's copy of the list; syncShuffling / putIndexList reach every GPU.
const assert = require("assert");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "bls_gpu_verifier.js"));

class MockBackend {
  constructor() {
    this.batches = [];
    this.lists = new Map();
  }
  async verifyRequests(batch) {
    this.batches.push(batch);
    const n = batch.requestOffsets.length - 1;
    return {valid: new Uint8Array(n).fill(1), errors: new Uint8Array(n), setStatus: new Uint8Array(0),
      batchRetries: 0, batchSigsSuccess: 0, deviceMs: 0, workerStartNs: 0, workerEndNs: 0};
  }
  async indexListShuffle(listId, active, seed) {
    assert(active instanceof Uint32Array && seed.length === 32);
    const out = Uint32Array.from(active).reverse();
    this.lists.set(listId, out);
    return out;
  }
  async indexListPut(listId, ix) {
    assert(ix instanceof Uint32Array);
    this.lists.set(listId, ix);
    return ix.length;
  }
  async close() {}
}

const R = new Uint8Array(32).fill(7);
const S = new Uint8Array(96).fill(9);
const seed = () => new Uint8Array(32);
let failed = 0;
async function test(name, fn) {
  try {
    await fn();
    console.log("ok   " + name);
  } catch (e) {
    failed++;
    console.log("FAIL " + name + ": " + (e && e.stack ? e.stack : e));
  }
}

(async () => {
  await test("descriptors for index keys and bits sets", async () => {
    const b = new MockBackend();
    const v = new V.BlsGpuVerifier({backends: [b], seedSource: seed});
    const sets = [
      {type: "single", pubkey: {index: 4}, signingRoot: R, signature: S},
      {type: "bits", list: 0, start: 32, length: 10, bits: new Uint8Array([5, 2, 0xff]), signingRoot: R, signature: S},
      {type: "aggregate", pubkeys: [{index: 9}, {index: 8}], signingRoot: R, signature: S},
      {type: "bits", list: 1, start: 0, length: 16, bits: new Uint8Array([1, 128]), signingRoot: R, signature: S},
    ];
    assert.strictEqual(await v.verifySignatureSets(sets), true);
    const batch = b.batches[b.batches.length - 1];
    assert.deepStrictEqual(Array.from(batch.setKeys),
      [0, 0, 4, 0, 0, 2, 0, 32, 10, 0, 1, 0, 0, 2, 0, 2, 1, 0, 16, 2]);
    assert.deepStrictEqual(Array.from(batch.keyPool), [9, 8]);
    assert.deepStrictEqual(Array.from(batch.keyBits), [5, 2, 1, 128]);  // ceil(length / 8) bytes each
    assert.deepStrictEqual(Array.from(batch.requestOffsets), [0, 4]);
    assert.strictEqual(batch.messages.length, 4 * 32);
    assert.deepStrictEqual(Array.from(batch.sigOffsets), [0, 96, 192, 288, 384]);
    assert(batch.pubkeyIndices === undefined && batch.pkOffsets === undefined && batch.pubkeys === undefined);
    await v.close();
  });

  await test("fallback to today's form for a key with bytes", async () => {
    const b = new MockBackend();
    const v = new V.BlsGpuVerifier({backends: [b], seedSource: seed});
    await v.putIndexList(3, [70, 71, 72, 73, 74, 75, 76, 77, 78, 79]);
    const sets = [
      {type: "bits", list: 3, start: 2, length: 6, bits: new Uint8Array([0x29]), signingRoot: R, signature: S},
      {type: "single", pubkey: new Uint8Array(96).fill(3), signingRoot: R, signature: S},
      {type: "single", pubkey: {index: 5}, signingRoot: R, signature: S},
    ];
    assert.strictEqual(V.packSetKeys([sets]), null);
    assert.strictEqual(await v.verifySignatureSets(sets), true);
    const batch = b.batches[b.batches.length - 1];
    assert(batch.setKeys === undefined);
    assert.deepStrictEqual(Array.from(batch.pubkeyIndices), [72, 75, 77, 0x80000000, 5]);
    assert.deepStrictEqual(Array.from(batch.pkOffsets), [0, 3, 4, 5]);
    assert.strictEqual(batch.pubkeys.length, 96);
    // a list that was never loaded cannot be expanded on the host
    const orphan = [{type: "bits", list: 6, start: 0, length: 4, bits: new Uint8Array([1]), signingRoot: R, signature: S},
      sets[1]];
    await assert.rejects(v.verifySignatureSets(orphan), /index list 6 is not loaded/);
    await v.close();
  });

  await test("packages without bits sets are packed as before", async () => {
    const b = new MockBackend();
    const v = new V.BlsGpuVerifier({backends: [b], seedSource: seed});
    await v.verifySignatureSets([{type: "single", pubkey: {index: 4}, signingRoot: R, signature: S},
      {type: "aggregate", pubkeys: [{index: 1}, {index: 2}], signingRoot: R, signature: S}]);
    const batch = b.batches[b.batches.length - 1];
    assert(batch.setKeys === undefined);
    assert.deepStrictEqual(Array.from(batch.pubkeyIndices), [4, 1, 2]);
    await v.close();
  });

  await test("syncShuffling and putIndexList reach every GPU", async () => {
    const bs = [new MockBackend(), new MockBackend()];
    const v = new V.BlsGpuVerifier({backends: bs, seedSource: seed});
    const out = await v.syncShuffling(1, [3, 4, 5], new Uint8Array(32));
    assert(out instanceof Uint32Array);
    assert.deepStrictEqual(Array.from(out), [5, 4, 3]);
    await v.putIndexList(2, new Uint32Array([9, 9]));
    for (const b of bs) {
      assert.deepStrictEqual(Array.from(b.lists.get(1)), [5, 4, 3]);
      assert.deepStrictEqual(Array.from(b.lists.get(2)), [9, 9]);
    }
    await v.close();
  });

  await test("a bits set needs ceil(length / 8) bytes", async () => {
    assert.throws(() => V.packSetKeys([[{type: "bits", list: 0, start: 0, length: 9, bits: new Uint8Array(1),
      signingRoot: R, signature: S}]]), /ceil\(length \/ 8\)/);
  });

  console.log(failed + " failed");
  process.exit(failed ? 1 : 0);
})();
