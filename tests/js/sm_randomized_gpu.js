"use strict";
// One same-message job (argv[2]: JSON {pks, sigs, root} in hex, 96-byte keys) through the real
// addon on GPU 0: with sameMessageRandomized, then with the default plain sums.  Prints
// {"randomized": [...], "plain": [...]} (the job's per-set verdicts) as its last line.
const fs = require("fs");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "bls_gpu_verifier.js"));

const hex = (s) => new Uint8Array(Buffer.from(s, "hex"));

async function main() {
  const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
  const sets = job.pks.map((p, i) => ({publicKey: hex(p), signature: hex(job.sigs[i])}));
  const root = hex(job.root);
  const seedSource = () => new Uint8Array(32).fill(7);
  const out = {};
  for (const [name, randomized] of [["randomized", true], ["plain", false]]) {
    const v = new V.BlsGpuVerifier({devices: [0], seedSource, sameMessageRandomized: randomized});
    if (v.backends[0].sameMessageRandomized !== randomized) throw new Error(`context mode of ${name}`);
    out[name] = await v.verifySignatureSetsSameMessage(sets, root);
    await v.close();
  }
  console.log(JSON.stringify(out));
}
main().catch((e) => {
  console.error(e && e.stack);
  process.exit(1);
});
