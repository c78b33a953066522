"use strict";
// Commitments and proofs of lodestar_amd/js/kzg.js through the real addon on the GPU.  argv[2]: a
// directory holding trusted_setup.txt (an honest Lagrange setup of a known tau) and blobs.bin /
// commitments.bin / proofs.bin of three honest sidecars, plus z.bin / y.bin / zproof.bin of
// computeKzgProof(blob 0, z) (written by tests/test_gpu_kzg_commit.py).
const assert = require("assert");
const fs = require("fs");
const path = require("path");
const K = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "kzg.js"));

function split(buf, size) {
  const out = [];
  for (let i = 0; i < buf.length; i += size) out.push(Uint8Array.from(buf.subarray(i, i + size)));
  return out;
}
const same = (a, b) => Buffer.from(a).equals(Buffer.from(b));

async function rejects(fn, re) {
  let err = null;
  try {
    await fn();
  } catch (e) {
    err = e;
  }
  assert.ok(err && re.test(err.message), err ? err.message : "expected a throw");
  return err;
}

async function main() {
  const dir = process.argv[2];
  const read = (name) => fs.readFileSync(path.join(dir, name));
  const blobs = split(read("blobs.bin"), K.BYTES_PER_BLOB);
  const coms = split(read("commitments.bin"), 48);
  const proofs = split(read("proofs.bin"), 48);
  const ctx = new (K.loadAddon().Context)(0);
  const kzg = K.createGpuKzg(ctx);
  const e = await rejects(() => ctx.kzgBlobCommitments(blobs[0]), /no G1 setup/);
  assert.strictEqual(e.code, "LB_ERR_INVALID_ARGUMENT");
  // a refused G1 setup names the line
  const text = fs.readFileSync(path.join(dir, "trusted_setup.txt"), "utf8");
  const g1 = K.parseTrustedSetupG1(text);
  const bad = Uint8Array.from(g1);
  bad[48 * 9] &= 0x7f;
  await rejects(() => ctx.kzgLoadSetupG1(bad), /G1 point 9 .*bad index 9/);
  await rejects(() => ctx.kzgBlobCommitments(blobs[0]), /no G1 setup/);

  await kzg.loadTrustedSetup(path.join(dir, "trusted_setup.txt"));
  const gotC = await kzg.blobsToKzgCommitments(blobs);
  assert.strictEqual(gotC.length, 3);
  gotC.forEach((c, i) => assert.ok(same(c, coms[i]), `commitment ${i}`));
  const gotP = await kzg.computeBlobKzgProofs(blobs, coms);
  gotP.forEach((p, i) => assert.ok(same(p, proofs[i]), `proof ${i}`));
  assert.ok(same(await kzg.blobToKzgCommitment(blobs[1]), coms[1]));
  assert.ok(same(await kzg.computeBlobKzgProof(blobs[2], coms[2]), proofs[2]));
  assert.strictEqual(await kzg.verifyBlobKzgProofBatch(blobs, gotC, gotP), true);
  const [zp, y] = await kzg.computeKzgProof(blobs[0], Uint8Array.from(read("z.bin")));
  assert.ok(same(zp, read("zproof.bin")) && same(y, read("y.bin")));
  // the raw entry: a bad item is zeroed, its neighbour exact
  const big = Uint8Array.from(blobs[0]);
  big.fill(0xff, 0, 32);
  const two = new Uint8Array(2 * K.BYTES_PER_BLOB);
  two.set(big, 0);
  two.set(blobs[1], K.BYTES_PER_BLOB);
  const raw = await ctx.kzgBlobCommitments(two);
  assert.deepStrictEqual(Array.from(raw.status), [1, 0]);
  assert.ok(raw.commitments.subarray(0, 48).every((x) => x === 0) && same(raw.commitments.subarray(48), coms[1]));
  await rejects(() => kzg.blobToKzgCommitment(big), /item 0: BAD_BLOB/);
  await rejects(() => kzg.computeBlobKzgProof(blobs[0], new Uint8Array(48)), /item 0: BAD_COMMITMENT/);
  await ctx.close();
  console.log("kzg commit gpu ok");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
