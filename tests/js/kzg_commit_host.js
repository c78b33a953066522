"use strict";
// lodestar_amd/js/kzg.js against a stand-in backend that HAS the commitment entries (no GPU, no
// addon): the G1 half of the trusted-setup parser, the load order, the shapes of the results, the
// split into device calls, and the throw side (lengths before the device, statuses after it).
const assert = require("assert");
const fs = require("fs");
const os = require("os");
const path = require("path");
const K = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "kzg.js"));

const hex = (n, v) => v.toString(16).padStart(2 * n, "0");
const g1 = Array.from({length: 4096}, (_, i) => hex(48, i + 1));
const g2 = Array.from({length: 65}, (_, i) => hex(96, 1000 + i));
const setupText = "4096\n65\n" + g1.join("\n") + "\n" + g2.join("\n") + "\n";

class Backend {
  constructor() {
    this.order = [];
    this.calls = [];
    this.status = null;
    this.failG1 = false;
  }
  async kzgLoadSetup(tau) {
    this.order.push("g2");
    this.tau = Buffer.from(tau).toString("hex");
  }
  async kzgLoadSetupG1(points) {
    if (this.failG1) throw Error("G1 point 7 of the file is not in G1 (bad index 7)");
    this.order.push("g1");
    this.g1 = points;
  }
  out(name, n, size, fill) {
    this.calls.push({name, n});
    return {[name]: new Uint8Array(n * size).fill(fill), status: this.status || new Uint8Array(n)};
  }
  async kzgBlobCommitments(blobs) {
    return this.out("commitments", blobs.length / K.BYTES_PER_BLOB, 48, 0xc1);
  }
  async kzgBlobProofs(blobs, commitments) {
    assert.strictEqual(commitments.length, (blobs.length / K.BYTES_PER_BLOB) * 48);
    return this.out("proofs", blobs.length / K.BYTES_PER_BLOB, 48, 0xc2);
  }
  async kzgComputeProofs(blobs, zs) {
    assert.strictEqual(zs.length, (blobs.length / K.BYTES_PER_BLOB) * 32);
    const r = this.out("proofs", blobs.length / K.BYTES_PER_BLOB, 48, 0xc3);
    r.ys = new Uint8Array(zs.length).fill(7);
    return r;
  }
}

async function rejects(fn, re) {
  let err = null;
  try {
    await fn();
  } catch (e) {
    err = e;
  }
  assert.ok(err, "expected a throw");
  assert.ok(re.test(err.message), err.message);
}

async function main() {
  const file = path.join(fs.mkdtempSync(path.join(os.tmpdir(), "kzg-")), "trusted_setup.txt");
  fs.writeFileSync(file, setupText);
  const points = K.parseTrustedSetupG1(setupText);
  assert.strictEqual(points.length, 196608);
  assert.strictEqual(Buffer.from(points).toString("hex"), g1.join(""));
  assert.throws(() => K.parseTrustedSetupG1("4096\n64\n"), /expected 4096 G1 and 65 G2/);
  assert.throws(() => K.parseTrustedSetupG1(setupText.replace(g1[5], g1[5].slice(2))), /G1 point 5 is not 48 hex bytes/);

  const b = new Backend();
  const kzg = K.createGpuKzg(b);
  for (const m of ["blobToKzgCommitment", "computeBlobKzgProof", "blobsToKzgCommitments", "computeBlobKzgProofs",
    "computeKzgProof"]) assert.strictEqual(typeof kzg[m], "function", m);
  const blob = new Uint8Array(K.BYTES_PER_BLOB).fill(7);
  const c48 = new Uint8Array(48).fill(1);
  const z32 = new Uint8Array(32).fill(2);
  await rejects(() => kzg.blobToKzgCommitment(blob), /not loaded/);
  // a refused G1 setup rejects with the index, leaves [tau]_2 unloaded and the object unloaded
  b.failG1 = true;
  await rejects(() => kzg.loadTrustedSetup(file), /bad index 7/);
  assert.deepStrictEqual(b.order, []);
  await rejects(() => kzg.blobToKzgCommitment(blob), /not loaded/);
  b.failG1 = false;
  await kzg.loadTrustedSetup(file);
  assert.deepStrictEqual(b.order, ["g1", "g2"]);
  assert.strictEqual(b.tau, g2[1]);
  assert.strictEqual(Buffer.from(b.g1).toString("hex"), g1.join(""));

  const com = await kzg.blobToKzgCommitment(blob);
  assert.ok(com instanceof Uint8Array && com.length === 48 && com.every((x) => x === 0xc1));
  const proof = await kzg.computeBlobKzgProof(blob, c48);
  assert.ok(proof instanceof Uint8Array && proof.length === 48 && proof.every((x) => x === 0xc2));
  const [p, y] = await kzg.computeKzgProof(blob, z32);
  assert.ok(p.length === 48 && p[0] === 0xc3 && y.length === 32 && y[0] === 7);
  assert.deepStrictEqual(await kzg.blobsToKzgCommitments([]), []);
  assert.deepStrictEqual(await kzg.computeBlobKzgProofs([], []), []);
  // more than one device call's worth is split; item numbers count through the parts
  b.calls = [];
  const many = Array.from({length: 66}, () => blob);
  assert.strictEqual((await kzg.blobsToKzgCommitments(many)).length, 66);
  assert.deepStrictEqual(b.calls, [{name: "commitments", n: 64}, {name: "commitments", n: 2}]);
  // malformed input never reaches the device
  b.calls = [];
  await rejects(() => kzg.blobToKzgCommitment(blob.subarray(1)), /blob 0: expected 131072 bytes/);
  await rejects(() => kzg.computeBlobKzgProof(blob, c48.subarray(1)), /commitment 0: expected 48 bytes/);
  await rejects(() => kzg.computeBlobKzgProofs([blob, blob], [c48]), /differ in length/);
  await rejects(() => kzg.computeKzgProof(blob, z32.subarray(1)), /z 0: expected 32 bytes/);
  assert.deepStrictEqual(b.calls, []);
  // a status throws, naming the item
  b.status = Uint8Array.from([0, 1]);
  await rejects(() => kzg.blobsToKzgCommitments([blob, blob]), /item 1: BAD_BLOB/);
  b.status = Uint8Array.from([2]);
  await rejects(() => kzg.computeBlobKzgProof(blob, c48), /item 0: BAD_COMMITMENT/);
  b.status = Uint8Array.from([4]);
  await rejects(() => kzg.computeKzgProof(blob, z32), /item 0: BAD_SCALAR/);
  console.log("kzg commit host ok");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
