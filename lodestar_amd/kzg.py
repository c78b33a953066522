"""c-kzg's blob surface on the GPU (``lb_kzg_*``).

``GpuKzg`` has the shape of the ``ckzg`` object the beacon node uses
(packages/beacon-node/src/util/kzg.ts:15-29) and keeps its split between throwing
and returning ``False``: malformed input (wrong lengths, a field element >= r, bytes
that are not a G1 point) raises, as c-kzg's C_KZG_BADARGS does; only a failed pairing
check returns ``False`` (chain/validation/blobSidecar.ts:207-216 reports the two
differently).  Commitments and proofs (``blob_to_kzg_commitment``, ``compute_blob_kzg_proof``,
``compute_kzg_proof``) run a fixed-base MSM over the setup's G1 Lagrange points; on a device
object without those entry points the two ckzg-shaped methods still say "use c-kzg".
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


def parse_trusted_setup_g1(text: str) -> bytes:
    """The 4096 G1 Lagrange points of a ``trusted_setup.txt``, 48 bytes each, in file order
    (KZG_SETUP_G1_LAGRANGE is their bit-reversal permutation; the device applies it)."""
    lines = text.split()
    parse_trusted_setup(text)  # (the counts and the line total)
    out = []
    for i, line in enumerate(lines[2:2 + SETUP_G1_POINTS]):
        try:
            p = bytes.fromhex(line)
        except ValueError as e:
            raise KzgError(f"trusted setup: G1 point {i} is not hex: {e}") from None
        if len(p) != BYTES_PER_G1:
            raise KzgError(f"trusted setup: G1 point {i} has {len(p)} bytes")
        out.append(p)
    return b"".join(out)


class GpuKzg:
    """The ``ckzg`` object's blob methods on one :class:`native.Device`."""

    def __init__(self, device: Optional[native.Device] = None):
        self.dev = device if device is not None else native.Device(0)
        self._loaded = False

    # -- setup ---------------------------------------------------------------
    def load_trusted_setup(self, path: str) -> None:
        if self._loaded:
            raise KzgError("Error trusted setup is already loaded")  # (util/kzg.ts:80 matches this text)
        with open(path) as f:
            text = f.read()
        tau = parse_trusted_setup(text)
        # G1 first: a refused G1 point leaves the device's [tau]_2 as it was
        if hasattr(self.dev, "kzg_load_setup_g1"):
            self.dev.kzg_load_setup_g1(parse_trusted_setup_g1(text))
        self.dev.kzg_load_setup(tau)
        self._loaded = True

    def free_trusted_setup(self) -> None:
        self._loaded = False

    # -- verification ------------------------------------------------------------
    def _raise_on_status(self, statuses, first: int = 0) -> None:
        for i, st in enumerate(statuses):
            if st != native.LB_KZG_OK:
                raise KzgError(f"item {first + i}: {native.KZG_STATUS_NAMES.get(st, st)}")

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

    # -- commitments and proofs -----------------------------------------------------
    def _need(self, method: str) -> None:
        if not hasattr(self.dev, method):
            raise NotImplementedError("not implemented: use c-kzg")
        if not self._loaded:
            raise KzgError("trusted setup is not loaded")

    @staticmethod
    def _lengths(name: str, items: Sequence[bytes], size: int) -> None:
        for i, x in enumerate(items):
            if len(x) != size:
                raise KzgError(f"{name} {i}: expected {size} bytes, got {len(x)}")

    def _in_parts(self, call, n_out: int, *columns):
        """call(columns[lo:hi]...) over parts of at most LB_KZG_MAX_BLOBS items -> its n_out output
        columns joined; a status raises."""
        outs = [[] for _ in range(n_out)]
        for lo in range(0, len(columns[0]), native.LB_KZG_MAX_BLOBS):
            res = call(*[c[lo:lo + native.LB_KZG_MAX_BLOBS] for c in columns])
            self._raise_on_status(res[-1], lo)
            for o, r in zip(outs, res[:n_out]):
                o.extend(r)
        return outs

    def blobs_to_kzg_commitments(self, blobs: Sequence[bytes]) -> list:
        self._need("kzg_blob_commitments")
        self._lengths("blob", blobs, BYTES_PER_BLOB)
        return self._in_parts(self.dev.kzg_blob_commitments, 1, list(blobs))[0]

    def blob_to_kzg_commitment(self, blob: bytes) -> bytes:
        return self.blobs_to_kzg_commitments([blob])[0]

    def compute_blob_kzg_proofs(self, blobs: Sequence[bytes], commitments: Sequence[bytes]) -> list:
        self._need("kzg_blob_proofs")
        if len(blobs) != len(commitments):
            raise KzgError("blobs and commitments differ in length")
        self._lengths("blob", blobs, BYTES_PER_BLOB)
        self._lengths("commitment", commitments, BYTES_PER_G1)
        return self._in_parts(self.dev.kzg_blob_proofs, 1, list(blobs), list(commitments))[0]

    def compute_blob_kzg_proof(self, blob: bytes, commitment: bytes) -> bytes:
        return self.compute_blob_kzg_proofs([blob], [commitment])[0]

    def compute_kzg_proof(self, blob: bytes, z: bytes):
        """-> (proof, y)"""
        self._need("kzg_compute_proofs")
        self._lengths("blob", [blob], BYTES_PER_BLOB)
        self._lengths("z", [z], 32)
        proofs, ys = self._in_parts(self.dev.kzg_compute_proofs, 2, [blob], [z])
        return proofs[0], ys[0]
