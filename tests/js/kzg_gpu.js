"use strict";
// lodestar_amd/js/kzg.js through the real addon on the GPU.  argv[2]: a directory holding
// trusted_setup.txt and blobs.bin / commitments.bin / proofs.bin of three honest sidecars
// (written by tests/test_gpu_kzg.py).
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const K = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "kzg.js"));

function split(buf, size) {
  const out = [];
  for (let i = 0; i < buf.length; i += size) out.push(Uint8Array.from(buf.subarray(i, i + size)));
  return out;
}

async function main() {
  const dir = process.argv[2];
  const blobs = split(fs.readFileSync(path.join(dir, "blobs.bin")), K.BYTES_PER_BLOB);
  const coms = split(fs.readFileSync(path.join(dir, "commitments.bin")), 48);
  const proofs = split(fs.readFileSync(path.join(dir, "proofs.bin")), 48);
  const ctx = new (K.loadAddon().Context)(0);
  const kzg = K.createGpuKzg(ctx);
  let threw = null;
  try {
    await ctx.kzgVerifyBlobProofBatch(new Uint8Array(K.BYTES_PER_BLOB), new Uint8Array(48), new Uint8Array(48));
  } catch (e) {
    threw = e;
  }
  assert.ok(threw && threw.code === "LB_ERR_INVALID_ARGUMENT" && /no trusted setup/.test(threw.message));
  await kzg.loadTrustedSetup(path.join(dir, "trusted_setup.txt"));
  assert.strictEqual(await kzg.verifyBlobKzgProofBatch(blobs, coms, proofs), true);
  assert.strictEqual(await kzg.verifyBlobKzgProof(blobs[0], coms[0], proofs[0]), true);
  assert.strictEqual(await kzg.verifyBlobKzgProof(blobs[0], coms[0], proofs[1]), false);
  assert.strictEqual(await kzg.verifyBlobKzgProofBatch(blobs, coms, [proofs[1], proofs[0], proofs[2]]), false);
  let bad = null;
  try {
    await kzg.verifyBlobKzgProof(blobs[0], coms[0], new Uint8Array(48));
  } catch (e) {
    bad = e;
  }
  assert.ok(bad && /BAD_PROOF/.test(bad.message));
  const big = Uint8Array.from(blobs[0]);
  big.fill(0xff, 0, 32);
  bad = null;
  try {
    await kzg.verifyBlobKzgProof(big, coms[0], proofs[0]);
  } catch (e) {
    bad = e;
  }
  assert.ok(bad && /BAD_BLOB/.test(bad.message));
  await ctx.close();
  console.log("kzg gpu ok");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
