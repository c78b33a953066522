"""Latency of blob KZG proof verification on one GPU: p50 over 20 calls of 1-, 6- and
9-blob verifyBlobKzgProofBatch (host buffers in, verdict out) and the three stage times
of the last call; and the same for blobToKzgCommitment and computeBlobKzgProof at 1 and 6
blobs (results checked against the known-tau expectation on every call), with the table-build
time of the G1 setup load.  A separate tool: bench.py measures the signature workload only.

Usage: python tools/kzg_probe.py [--calls 20] [--device 0]
Prints one JSON line.  The sidecars are honest ones under a test setup with a known tau
(tests/kzg_helper.py), so the verdict is checked on every call.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lodestar_amd.native import Device  # noqa: E402
from tests import kzg_commit_helper as C  # noqa: E402
from tests import kzg_helper as K  # noqa: E402


def timed(calls, fn, want):
    for _ in range(3):  # warm-up: code objects, workspace, clocks
        assert fn() == want
    wall = []
    for _ in range(calls):
        t0 = time.perf_counter()
        got = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
        assert got == want
    return wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    setup = K.TestSetup()
    sidecars = [setup.blob_case(K.random_poly(900 + i))[:3] for i in range(9)]
    dev = Device(args.device)
    dev.kzg_load_setup(setup.tau_g2)
    out = {"calls": args.calls, "sizes": {}}
    for n in (1, 6, 9):
        blobs, coms, proofs = ([s[k] for s in sidecars[:n]] for k in range(3))
        for _ in range(3):  # warm-up: code objects, workspace, clocks
            assert dev.kzg_verify_blob_proof_batch(blobs, coms, proofs)[0]
        wall = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            ok, _ = dev.kzg_verify_blob_proof_batch(blobs, coms, proofs)
            wall.append((time.perf_counter() - t0) * 1e3)
            assert ok
        out["sizes"][str(n)] = {
            "p50_ms": round(statistics.median(wall), 3), "min_ms": round(min(wall), 3), "max_ms": round(max(wall), 3),
            "stages_ms": {k: round(v, 3) for k, v in dev.last_stage_times()},
        }
    # commitments and proofs: an honest Lagrange setup of the same tau, its points made on the GPU
    pks = dev.sk_to_pk([x.to_bytes(32, "big") for x in C.lagrange_scalars(setup.tau)])
    g1 = b"".join(C.file_order([C.g1_compress(p) for p in pks]))
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        dev.kzg_load_setup_g1(g1)
        wall.append((time.perf_counter() - t0) * 1e3)
    out["load_setup_g1"] = {"wall_ms": [round(w, 3) for w in wall],
                            "stages_ms": {k: round(v, 3) for k, v in dev.last_stage_times()}}
    for name in ("commitments", "proofs"):
        out[name] = {}
        for n in (1, 6):
            blobs, coms, proofs = ([s[k] for s in sidecars[:n]] for k in range(3))
            if name == "commitments":
                wall = timed(args.calls, lambda: dev.kzg_blob_commitments(blobs), (coms, [0] * n))
            else:
                wall = timed(args.calls, lambda: dev.kzg_blob_proofs(blobs, coms), (proofs, [0] * n))
            out[name][str(n)] = {
                "p50_ms": round(statistics.median(wall), 3), "min_ms": round(min(wall), 3),
                "max_ms": round(max(wall), 3), "stages_ms": {k: round(v, 3) for k, v in dev.last_stage_times()},
            }
    dev.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
