"use strict";
// c-kzg's blob surface on the GPU: an object of the shape of `ckzg` in
// packages/beacon-node/src/util/kzg.ts:15-22, over an addon Context
// (kzgLoadSetup / kzgVerifyBlobProofBatch / kzgLoadSetupG1 / kzgBlobCommitments / kzgBlobProofs /
// kzgComputeProofs -> lb_kzg_*).
//
// The split between throwing and returning false is c-kzg's: malformed input -- wrong
// lengths, a field element >= r, bytes that are not a point of G1 (C_KZG_BADARGS) --
// throws; only a failed pairing check gives false
// (chain/validation/blobSidecar.ts:207-216 reports the two differently).
//
// One difference: the addon never blocks the event loop, so loadTrustedSetup, the two verify
// methods and blobToKzgCommitment / computeBlobKzgProof / computeKzgProof return Promises
// (c-kzg's are synchronous on the main thread) -- the call sites add an `await`.  On a backend
// without the commitment entries the two compute methods throw "not implemented: use c-kzg",
// synchronously.
const fs = require("fs");
const path = require("path");

const BYTES_PER_BLOB = 131072;
const BYTES_PER_G1 = 48;
const BYTES_PER_G2 = 96;
const BYTES_PER_FIELD_ELEMENT = 32;
const SETUP_G1_POINTS = 4096;
const MAX_BLOBS_PER_CALL = 64; // LB_KZG_MAX_BLOBS
const STATUS_NAMES = ["OK", "BAD_BLOB", "BAD_COMMITMENT", "BAD_PROOF", "BAD_SCALAR"];

// KZG_SETUP_G2_MONOMIAL[1] of a trusted_setup.txt: count lines 4096 and 65, 4096 G1 lines,
// 65 G2 lines; the verifier needs G2 line index 1 alone
function parseTrustedSetup(text) {
  const lines = text.split(/\s+/).filter((x) => x.length > 0);
  const n1 = Number(lines[0]);
  const n2 = Number(lines[1]);
  if (n1 !== 4096 || n2 !== 65) throw Error(`trusted setup: expected 4096 G1 and 65 G2 points, got ${lines[0]}, ${lines[1]}`);
  if (lines.length !== 2 + n1 + n2) throw Error(`trusted setup: expected ${2 + n1 + n2} lines, got ${lines.length}`);
  const hex = lines[2 + n1 + 1];
  if (!/^[0-9a-fA-F]+$/.test(hex) || hex.length !== 2 * BYTES_PER_G2) throw Error("trusted setup: G2 point 1 is not 96 hex bytes");
  return Uint8Array.from(Buffer.from(hex, "hex"));
}

// The 4096 G1 Lagrange lines of a trusted_setup.txt, 48 bytes each, in file order (the device
// applies the bit-reversal permutation of KZG_SETUP_G1_LAGRANGE)
function parseTrustedSetupG1(text) {
  parseTrustedSetup(text); // (the counts and the line total)
  const lines = text.split(/\s+/).filter((x) => x.length > 0);
  const out = new Uint8Array(SETUP_G1_POINTS * BYTES_PER_G1);
  for (let i = 0; i < SETUP_G1_POINTS; i++) {
    const hex = lines[2 + i];
    if (!/^[0-9a-fA-F]+$/.test(hex) || hex.length !== 2 * BYTES_PER_G1) throw Error(`trusted setup: G1 point ${i} is not 48 hex bytes`);
    out.set(Buffer.from(hex, "hex"), i * BYTES_PER_G1);
  }
  return out;
}

function split(buf, size, n) {
  return Array.from({length: n}, (_, i) => Uint8Array.from(buf.subarray(i * size, (i + 1) * size)));
}

function concat(items, size, what) {
  const out = new Uint8Array(items.length * size);
  items.forEach((x, i) => {
    if (!(x instanceof Uint8Array) || x.length !== size) throw Error(`${what} ${i}: expected ${size} bytes`);
    out.set(x, i * size);
  });
  return out;
}

// backend: an addon Context (or anything with its two kzg methods)
function createGpuKzg(backend) {
  let loaded = false;
  async function verifyBlobKzgProofBatch(blobs, expectedKzgCommitments, kzgProofs) {
    if (!loaded) throw Error("trusted setup is not loaded");
    if (blobs.length !== expectedKzgCommitments.length || blobs.length !== kzgProofs.length) {
      throw Error("blobs, commitments and proofs differ in length");
    }
    let ok = true;
    for (let lo = 0; lo < blobs.length; lo += MAX_BLOBS_PER_CALL) {
      const hi = Math.min(blobs.length, lo + MAX_BLOBS_PER_CALL);
      const res = await backend.kzgVerifyBlobProofBatch(
        concat(blobs.slice(lo, hi), BYTES_PER_BLOB, "blob"),
        concat(expectedKzgCommitments.slice(lo, hi), BYTES_PER_G1, "commitment"),
        concat(kzgProofs.slice(lo, hi), BYTES_PER_G1, "proof")
      );
      res.status.forEach((st, i) => {
        if (st !== 0) throw Error(`item ${lo + i}: ${STATUS_NAMES[st] || st}`);
      });
      ok = ok && res.ok === true;
    }
    return ok;
  }
  // The commitment / proof methods.  The check for the backend's entry is synchronous (a backend
  // without it throws, it does not reject); lengths and statuses reject before / after the device.
  function need(method) {
    if (typeof backend[method] !== "function") throw Error("not implemented: use c-kzg");
  }
  // columns: [items, size, name]...; call(joined columns...) per part of at most MAX_BLOBS_PER_CALL
  // items -> the named output columns, split per item
  async function inParts(method, columns, outputs) {
    if (!loaded) throw Error("trusted setup is not loaded");
    const n = columns[0][0].length;
    for (const [items] of columns) if (items.length !== n) throw Error("blobs and their companions differ in length");
    const joined = [];
    for (let lo = 0; lo < n; lo += MAX_BLOBS_PER_CALL) {
      const hi = Math.min(n, lo + MAX_BLOBS_PER_CALL);
      joined.push(columns.map(([items, size, what]) => concat(items.slice(lo, hi), size, what)));
    }
    const out = outputs.map(() => []);
    for (let k = 0; k < joined.length; k++) {
      const res = await backend[method](...joined[k]);
      res.status.forEach((st, i) => {
        if (st !== 0) throw Error(`item ${k * MAX_BLOBS_PER_CALL + i}: ${STATUS_NAMES[st] || st}`);
      });
      outputs.forEach(([name, size], j) => out[j].push(...split(res[name], size, res.status.length)));
    }
    return out;
  }
  function blobsToKzgCommitments(blobs) {
    need("kzgBlobCommitments");
    return inParts("kzgBlobCommitments", [[blobs, BYTES_PER_BLOB, "blob"]], [["commitments", BYTES_PER_G1]]).then((o) => o[0]);
  }
  function computeBlobKzgProofs(blobs, commitments) {
    need("kzgBlobProofs");
    return inParts("kzgBlobProofs", [[blobs, BYTES_PER_BLOB, "blob"], [commitments, BYTES_PER_G1, "commitment"]],
      [["proofs", BYTES_PER_G1]]).then((o) => o[0]);
  }
  return {
    async loadTrustedSetup(filePath) {
      if (loaded) throw Error("Error trusted setup is already loaded"); // (util/kzg.ts:80 matches this text)
      const text = fs.readFileSync(filePath, "utf8");
      const tau = parseTrustedSetup(text);
      // G1 first: a refused G1 point leaves the backend's [tau]_2 as it was
      if (typeof backend.kzgLoadSetupG1 === "function") await backend.kzgLoadSetupG1(parseTrustedSetupG1(text));
      await backend.kzgLoadSetup(tau);
      loaded = true;
    },
    freeTrustedSetup() {
      loaded = false;
    },
    blobToKzgCommitment(blob) {
      need("kzgBlobCommitments");
      return blobsToKzgCommitments([blob]).then((c) => c[0]);
    },
    computeBlobKzgProof(blob, commitment) {
      need("kzgBlobProofs");
      return computeBlobKzgProofs([blob], [commitment]).then((p) => p[0]);
    },
    blobsToKzgCommitments,
    computeBlobKzgProofs,
    // -> [proof, y], as c-kzg's computeKzgProof
    computeKzgProof(blob, z) {
      need("kzgComputeProofs");
      return inParts("kzgComputeProofs", [[[blob], BYTES_PER_BLOB, "blob"], [[z], BYTES_PER_FIELD_ELEMENT, "z"]],
        [["proofs", BYTES_PER_G1], ["ys", BYTES_PER_FIELD_ELEMENT]]).then(([p, y]) => [p[0], y[0]]);
    },
    verifyBlobKzgProof(blob, commitment, proof) {
      return verifyBlobKzgProofBatch([blob], [commitment], [proof]);
    },
    verifyBlobKzgProofBatch,
  };
}

function loadAddon() {
  return require(path.join(__dirname, "..", "napi", "lodestar_bls.node"));
}

module.exports = {createGpuKzg, parseTrustedSetup, parseTrustedSetupG1, loadAddon, BYTES_PER_BLOB, BYTES_PER_G1, BYTES_PER_G2, STATUS_NAMES};
