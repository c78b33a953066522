"""c-kzg's verification surface on the GPU (``lb_kzg_*``).

``GpuKzg`` has the shape of the ``ckzg`` object the beacon node uses
(packages/beacon-node/src/util/kzg.ts:15-29) and keeps its split between throwing
and returning ``False``: malformed input (wrong lengths, a field element >= r, bytes
that are not a G1 point) raises, as c-kzg's C_KZG_BADARGS does; only a failed pairing
check returns ``False`` (chain/validation/blobSidecar.ts:207-216 reports the two
differently).  Commitments and proofs are not computed here.
"""
from __future__ import annotations

from typing import Optional, Sequence

from . import native

BYTES_PER_BLOB = native.LB_KZG_BLOB_BYTES
BYTES_PER_G1 = 48
BYTES_PER_G2 = 96
SETUP_G1_POINTS = 4096
SETUP_G2_POINTS = 65


class KzgError(native.LodestarBlsError):
    pass


def parse_trusted_setup(text: str) -> bytes:
    """KZG_SETUP_G2_MONOMIAL[1] of a ``trusted_setup.txt``: two count lines (4096, 65),
    4096 G1 lines, 65 G2 lines, hex; the verifier needs only [tau]_2, G2 line index 1."""
    lines = text.split()
    if len(lines) < 2 or not lines[0].isdigit() or not lines[1].isdigit():
        raise KzgError("trusted setup: missing point counts")
    n1, n2 = int(lines[0]), int(lines[1])
    if n1 != SETUP_G1_POINTS or n2 != SETUP_G2_POINTS:
        raise KzgError(f"trusted setup: expected {SETUP_G1_POINTS} G1 and {SETUP_G2_POINTS} G2 points, got {n1}, {n2}")
    if len(lines) != 2 + n1 + n2:
        raise KzgError(f"trusted setup: expected {2 + n1 + n2} lines, got {len(lines)}")
    try:
        tau = bytes.fromhex(lines[2 + n1 + 1])
    except ValueError as e:
        raise KzgError(f"trusted setup: G2 point 1 is not hex: {e}") from None
    if len(tau) != BYTES_PER_G2:
        raise KzgError(f"trusted setup: G2 point 1 has {len(tau)} bytes")
    return tau


class GpuKzg:
    """verifyBlobKzgProof / verifyBlobKzgProofBatch on one :class:`native.Device`."""

    def __init__(self, device: Optional[native.Device] = None):
        self.dev = device if device is not None else native.Device(0)
        self._loaded = False

    # -- setup ---------------------------------------------------------------
    def load_trusted_setup(self, path: str) -> None:
        if self._loaded:
            raise KzgError("Error trusted setup is already loaded")  # (util/kzg.ts:80 matches this text)
        with open(path) as f:
            tau = parse_trusted_setup(f.read())
        self.dev.kzg_load_setup(tau)
        self._loaded = True

    def free_trusted_setup(self) -> None:
        self._loaded = False

    # -- verification ------------------------------------------------------------
    def _raise_on_status(self, statuses) -> None:
        for i, st in enumerate(statuses):
            if st != native.LB_KZG_OK:
                raise KzgError(f"item {i}: {native.KZG_STATUS_NAMES.get(st, st)}")

    def verify_blob_kzg_proof_batch(self, blobs: Sequence[bytes], commitments: Sequence[bytes],
                                    proofs: Sequence[bytes]) -> bool:
        if not self._loaded:
            raise KzgError("trusted setup is not loaded")
        if len(blobs) != len(commitments) or len(blobs) != len(proofs):
            raise KzgError("blobs, commitments and proofs differ in length")
        for name, items, size in (("blob", blobs, BYTES_PER_BLOB), ("commitment", commitments, BYTES_PER_G1),
                                  ("proof", proofs, BYTES_PER_G1)):
            for i, x in enumerate(items):
                if len(x) != size:
                    raise KzgError(f"{name} {i}: expected {size} bytes, got {len(x)}")
        ok = True
        for lo in range(0, len(blobs), native.LB_KZG_MAX_BLOBS):  # (a block has at most 6)
            hi = lo + native.LB_KZG_MAX_BLOBS
            part_ok, st = self.dev.kzg_verify_blob_proof_batch(blobs[lo:hi], commitments[lo:hi], proofs[lo:hi])
            self._raise_on_status(st)
            ok = ok and part_ok
        return ok

    def verify_blob_kzg_proof(self, blob: bytes, commitment: bytes, proof: bytes) -> bool:
        return self.verify_blob_kzg_proof_batch([blob], [commitment], [proof])

    # -- not provided --------------------------------------------------------------
    def blob_to_kzg_commitment(self, blob: bytes) -> bytes:
        raise NotImplementedError("not implemented: use c-kzg")

    def compute_blob_kzg_proof(self, blob: bytes, commitment: bytes) -> bytes:
        raise NotImplementedError("not implemented: use c-kzg")
