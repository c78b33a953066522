"use strict";
// sameMessageRandomized reaches the addon Context through BlsGpuVerifier and
// BlsGpuSingleThreadVerifier (a stand-in addon module that records how its contexts are
// created; no GPU), and same-message jobs still flow through those contexts.
const assert = require("assert");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "bls_gpu_verifier.js"));

const created = [];
class MockContext {
  constructor(device, opts) {
    this.device = device;
    this.opts = opts;
    this.capacity = (opts && opts.capacity) || 2;
    this.sameMessageRandomized = Boolean(opts && opts.sameMessageRandomized);
    created.push(this);
  }
  async verifySameMessage(b) {
    const nJobs = b.jobOffsets.length - 1;
    const nSets = b.jobOffsets[nJobs];
    return {valid: new Uint8Array(nSets).fill(1), jobFast: new Uint8Array(nJobs).fill(1), retriedJobs: 0,
            fastSets: nSets, deviceMs: 0};
  }
  async close() {}
}
const addon = {Context: MockContext};

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
  const sets = [0, 1].map(() => ({publicKey: new Uint8Array(96), signature: new Uint8Array(96).fill(1)}));
  const root = new Uint8Array(32);

  await check("pool: the option reaches every context", async () => {
    created.length = 0;
    const v = new V.BlsGpuVerifier({addon, devices: [0, 1], capacity: 3, sameMessageRandomized: true});
    assert.strictEqual(created.length, 2);
    for (const c of created) assert.deepStrictEqual(c.opts, {capacity: 3, sameMessageRandomized: true});
    assert.strictEqual(v.sameMessageRandomized, true);
    assert.deepStrictEqual(await v.verifySignatureSetsSameMessage(sets, root), [true, true]);
    await v.close();
  });
  await check("pool: the default leaves the library's mode", async () => {
    created.length = 0;
    const v = new V.BlsGpuVerifier({addon});
    assert.strictEqual(created.length, 1);
    assert.deepStrictEqual(created[0].opts, {});
    assert.strictEqual(v.sameMessageRandomized, false);
    await v.close();
  });
  await check("single thread: the option reaches its context", async () => {
    created.length = 0;
    const v = new V.BlsGpuSingleThreadVerifier({addon, device: 1, sameMessageRandomized: true});
    assert.strictEqual(created.length, 1);
    assert.strictEqual(created[0].device, 1);
    assert.deepStrictEqual(created[0].opts, {sameMessageRandomized: true});
    assert.deepStrictEqual(await v.verifySignatureSetsSameMessage(sets, root), [true, true]);
    await v.close();
    created.length = 0;
    const w = new V.BlsGpuSingleThreadVerifier({addon});
    assert.deepStrictEqual(created[0].opts, {});
    await w.close();
  });
  console.log(`${failed} failed`);
  process.exit(failed ? 1 : 0);
}
main();
