"use strict";
// One same-message job (argv[2]: JSON {pks, sigs, root, include} in hex, 96-byte keys) through
// the real addon on GPU 0: verifyAndAggregateSameMessage on the pool verifier (all sets, then
// with `include`), on the single-thread verifier, and aggregateSignatureGroups over the job's
// signatures `groups` (index lists).  Prints {"all", "masked", "single", "groups"} as its last line.
const fs = require("fs");
const path = require("path");
const V = require(path.join(__dirname, "..", "..", "lodestar_amd", "js", "bls_gpu_verifier.js"));

const hex = (s) => new Uint8Array(Buffer.from(s, "hex"));
const show = (r) => ({valid: r.valid, signature: r.signature && Buffer.from(r.signature).toString("hex"), count: r.count});

async function main() {
  const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
  const sets = job.pks.map((p, i) => ({publicKey: hex(p), signature: hex(job.sigs[i])}));
  const root = hex(job.root);
  const seedSource = () => new Uint8Array(32).fill(7);
  const out = {};
  const v = new V.BlsGpuVerifier({devices: [0], seedSource});
  out.all = show(await v.verifyAndAggregateSameMessage(sets, root));
  out.masked = show(await v.verifyAndAggregateSameMessage(sets, root, {include: job.include}));
  out.plain = await v.verifySignatureSetsSameMessage(sets, root);
  const groups = job.groups.map((g) => g.map((i) => sets[i].signature));
  out.groups = (await v.aggregateSignatureGroups(groups)).map((s) => Buffer.from(s).toString("hex"));
  await v.close();
  const s = new V.BlsGpuSingleThreadVerifier({device: 0, seedSource});
  out.single = show(await s.verifyAndAggregateSameMessage(sets, root, {include: job.include}));
  await s.close();
  console.log(JSON.stringify(out));
}
main().catch((e) => {
  console.error(e && e.stack);
  process.exit(1);
});
