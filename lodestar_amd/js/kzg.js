"use strict";
// c-kzg's verification surface on the GPU: an object of the shape of `ckzg` in
// packages/beacon-node/src/util/kzg.ts:15-22, over an addon Context
// (kzgLoadSetup / kzgVerifyBlobProofBatch -> lb_kzg_*).
//
// The split between throwing and returning false is c-kzg's: malformed input -- wrong
// lengths, a field element >= r, bytes that are not a point of G1 (C_KZG_BADARGS) --
// throws; only a failed pairing check gives false
// (chain/validation/blobSidecar.ts:207-216 reports the two differently).
//
// One difference: the addon never blocks the event loop, so loadTrustedSetup and the two
// verify methods return Promises (c-kzg's are synchronous on the main thread) -- the
// call sites add an `await`.  blobToKzgCommitment / computeBlobKzgProof are not provided.
const fs = require("fs");
const path = require("path");

const BYTES_PER_BLOB = 131072;
const BYTES_PER_G1 = 48;
const BYTES_PER_G2 = 96;
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
  return {
    async loadTrustedSetup(filePath) {
      if (loaded) throw Error("Error trusted setup is already loaded"); // (util/kzg.ts:80 matches this text)
      await backend.kzgLoadSetup(parseTrustedSetup(fs.readFileSync(filePath, "utf8")));
      loaded = true;
    },
    freeTrustedSetup() {
      loaded = false;
    },
    blobToKzgCommitment() {
      throw Error("not implemented: use c-kzg");
    },
    computeBlobKzgProof() {
      throw Error("not implemented: use c-kzg");
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

module.exports = {createGpuKzg, parseTrustedSetup, loadAddon, BYTES_PER_BLOB, BYTES_PER_G1, BYTES_PER_G2, STATUS_NAMES};
