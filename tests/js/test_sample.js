"use strict";
// syncBalances / computeProposers / syncCommittee on the JS host with a mock backend (no GPU):
// the slot seeds are SHA256(epochSeed || LE64(slot)), proposers ask for one place per seed among
// n candidates and map 0xFFFFFFFF to -1, the committee is stored, comes back with its aggregate
// key and is known to the host's copy of the lists; an unfilled committee rejects.
const assert = require("assert");
const crypto = require("crypto");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "bls_gpu_verifier.js"));

class MockBackend {
  constructor(found) {
    this.samples = [];
    this.balances = [];
    this.found = found;
  }
  async balanceTablePut(first, inc) {
    assert(inc instanceof Uint8Array);
    this.balances.push([first, Array.from(inc)]);
    return first + inc.length;
  }
  async sampleByBalance(req) {
    assert(req.seeds instanceof Uint8Array && req.activeIndices instanceof Uint32Array);
    this.samples.push(req);
    const ns = req.seeds.length / 32;
    const indices = new Uint32Array(ns * req.count);
    for (let i = 0; i < indices.length; i++) indices[i] = Math.floor(i / req.count) % 2 ? 0xffffffff : 100 + i;
    const found = new Uint32Array(ns).fill(this.found === undefined ? req.count : this.found);
    const out = {indices, found, tried: new Uint32Array(ns).fill(1)};
    if (req.aggregate && found[0] === req.count) out.aggregatePubkey = new Uint8Array(96).fill(req.storeList);
    return out;
  }
  async close() {}
}

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
  await test("computeProposers ships the slot seeds", async () => {
    const b = new MockBackend();
    const v = new V.BlsGpuVerifier({backends: [b, new MockBackend()], seedSource: seed});
    const epochSeed = Uint8Array.from({length: 32}, (_, i) => i);
    const got = await v.computeProposers(epochSeed, 64, [9, 8, 7, 6, 5]);
    const req = b.samples[b.samples.length - 1];
    assert.strictEqual(req.seeds.length, 32 * 32);
    for (const i of [0, 1, 31]) {
      const le = Buffer.alloc(8);
      le.writeBigUInt64LE(BigInt(64 + i));
      const want = crypto.createHash("sha256").update(epochSeed).update(le).digest();
      assert.deepStrictEqual(Buffer.from(req.seeds.subarray(32 * i, 32 * i + 32)), want);
    }
    assert.deepStrictEqual([req.count, req.maxIncrement, req.maxCandidates, req.storeList], [1, 32, 5, undefined]);
    assert.deepStrictEqual(Array.from(req.activeIndices), [9, 8, 7, 6, 5]);
    assert.deepStrictEqual(got, Array.from({length: 32}, (_, i) => (i % 2 ? -1 : 100 + i)));
    assert.strictEqual(v.backends[1].samples.length, 0);  // one GPU computes them
    assert.strictEqual((await v.computeProposers(epochSeed, 0, new Uint32Array([1, 2]), 4)).length, 4);
    await v.close();
  });

  await test("syncCommittee stores the list on every GPU and returns the aggregate", async () => {
    const bs = [new MockBackend(), new MockBackend()];
    const v = new V.BlsGpuVerifier({backends: bs, seedSource: seed});
    const s = new Uint8Array(32).fill(3);
    const r = await v.syncCommittee(5, [4, 5, 6], s);
    for (const b of bs) {
      const req = b.samples[0];
      assert.deepStrictEqual([req.count, req.maxIncrement, req.maxCandidates, req.storeList, req.aggregate],
        [512, 32, 4194304, 5, true]);
      assert.deepStrictEqual(Array.from(req.seeds), Array.from(s));
    }
    assert(r.indices instanceof Uint32Array && r.indices.length === 512 && r.indices[511] === 611);
    assert.deepStrictEqual(Array.from(r.aggregatePubkey), new Array(96).fill(5));
    assert.deepStrictEqual(Array.from(v.keyMap.lbLists.get(5)), Array.from(r.indices));
    await v.close();
  });

  await test("an unfilled committee rejects", async () => {
    const v = new V.BlsGpuVerifier({backends: [new MockBackend(511)], seedSource: seed});
    await assert.rejects(v.syncCommittee(5, [4, 5, 6], new Uint8Array(32), 512, 32, 1000), /not filled: 511 of 512/);
    assert(!(v.keyMap.lbLists && v.keyMap.lbLists.has(5)));
    await v.close();
  });

  await test("syncBalances forwards first to every GPU", async () => {
    const bs = [new MockBackend(), new MockBackend()];
    const v = new V.BlsGpuVerifier({backends: bs, seedSource: seed});
    assert.strictEqual(await v.syncBalances([32, 31, 0], 7), 10);
    assert.strictEqual(await v.syncBalances(new Uint8Array([1])), 1);
    for (const b of bs) assert.deepStrictEqual(b.balances, [[7, [32, 31, 0]], [0, [1]]]);
    await v.close();
  });

  await test("the single-thread verifier has the same calls", async () => {
    const b = new MockBackend();
    const v = new V.BlsGpuSingleThreadVerifier({backend: b, seedSource: seed});
    assert.strictEqual(await v.syncBalances([5, 6], 2), 4);
    assert.deepStrictEqual(await v.computeProposers(new Uint8Array(32), 3, [1, 2, 3], 2), [100, -1]);
    const r = await v.syncCommittee(1, [1, 2, 3], new Uint8Array(32), 4);
    assert.deepStrictEqual(Array.from(r.indices), [100, 101, 102, 103]);
    assert.strictEqual(b.samples[1].storeList, 1);
  });

  console.log(failed + " failed");
  process.exit(failed ? 1 : 0);
})();
