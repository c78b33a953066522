"use strict";
// lodestar_amd/js/kzg.js against a stand-in backend (no GPU, no addon): the shape of the
// ckzg object, the trusted-setup parser, and the split between throwing and false.
const assert = require("assert");
const fs = require("fs");
const os = require("os");
const path = require("path");
const K = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "kzg.js"));

const hex = (n, v) => v.toString(16).padStart(2 * n, "0");
const g2 = Array.from({length: 65}, (_, i) => hex(96, 1000 + i));
const setupText = "4096\n65\n" + Array.from({length: 4096}, (_, i) => hex(48, i + 1)).join("\n") + "\n" + g2.join("\n") + "\n";

class Backend {
  constructor() {
    this.loaded = null;
    this.calls = [];
    this.next = {ok: true, status: null};
  }
  async kzgLoadSetup(tau) {
    this.loaded = Buffer.from(tau).toString("hex");
  }
  async kzgVerifyBlobProofBatch(blobs, commitments, proofs) {
    const n = blobs.length / K.BYTES_PER_BLOB;
    this.calls.push({n, c: commitments.length, p: proofs.length, first: blobs[0]});
    return {ok: this.next.ok, status: this.next.status || new Uint8Array(n)};
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
  const b = new Backend();
  const kzg = K.createGpuKzg(b);
  for (const m of ["freeTrustedSetup", "loadTrustedSetup", "blobToKzgCommitment", "computeBlobKzgProof",
    "verifyBlobKzgProof", "verifyBlobKzgProofBatch"]) assert.strictEqual(typeof kzg[m], "function", m);
  const blob = new Uint8Array(K.BYTES_PER_BLOB).fill(7);
  const g1 = new Uint8Array(48).fill(1);
  await rejects(() => kzg.verifyBlobKzgProof(blob, g1, g1), /not loaded/);
  assert.deepStrictEqual(Buffer.from(K.parseTrustedSetup(setupText)).toString("hex"), g2[1]);
  assert.throws(() => K.parseTrustedSetup("4096\n64\n"), /expected 4096 G1 and 65 G2/);
  await kzg.loadTrustedSetup(file);
  assert.strictEqual(b.loaded, g2[1]);
  await rejects(() => kzg.loadTrustedSetup(file), /^Error trusted setup is already loaded$/);
  kzg.freeTrustedSetup();
  await kzg.loadTrustedSetup(file);

  assert.strictEqual(await kzg.verifyBlobKzgProofBatch([blob, blob], [g1, g1], [g1, g1]), true);
  assert.deepStrictEqual(b.calls.pop(), {n: 2, c: 96, p: 96, first: 7});
  assert.strictEqual(await kzg.verifyBlobKzgProofBatch([], [], []), true);
  b.next = {ok: false, status: null};
  assert.strictEqual(await kzg.verifyBlobKzgProof(blob, g1, g1), false); // a failed pairing: false
  b.next = {ok: false, status: Uint8Array.from([0, 3])};
  await rejects(() => kzg.verifyBlobKzgProofBatch([blob, blob], [g1, g1], [g1, g1]), /item 1: BAD_PROOF/);
  b.next = {ok: true, status: null};
  const before = b.calls.length;
  await rejects(() => kzg.verifyBlobKzgProofBatch([blob], [g1, g1], [g1]), /differ in length/);
  await rejects(() => kzg.verifyBlobKzgProof(blob.subarray(1), g1, g1), /blob 0: expected 131072 bytes/);
  await rejects(() => kzg.verifyBlobKzgProof(blob, g1.subarray(1), g1), /commitment 0: expected 48 bytes/);
  assert.strictEqual(b.calls.length, before); // malformed input never reaches the device
  assert.throws(() => kzg.blobToKzgCommitment(blob), /not implemented: use c-kzg/);
  assert.throws(() => kzg.computeBlobKzgProof(blob, g1), /not implemented: use c-kzg/);
  console.log("kzg host ok");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
