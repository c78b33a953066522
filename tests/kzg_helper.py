"""Blob KZG verification restated on Python integers and the oracle's curve (consensus-specs
deneb polynomial-commitments.md), plus a test setup whose tau is known.

With tau known, a commitment is [f(tau)]G1 and a proof [(f(tau) - y) / (tau - z)]G1: one
scalar multiplication each, so the tests know every expected verdict by construction.
No c-kzg source or vector is involved; the two domain strings are the spec text's.
"""
from __future__ import annotations

import hashlib
import random

from oracle import bls12_381 as O

R = O.R
N = 4096
BYTES_PER_BLOB = 32 * N
FS_DOMAIN = b"FSBLOBVERIFY_V1_"
RC_DOMAIN = b"RCKZGBATCH___V1_"
G1_INF = b"\xc0" + bytes(47)
assert len(FS_DOMAIN) == 16 and len(RC_DOMAIN) == 16

OMEGA = pow(7, (R - 1) // N, R)


def brp(i: int, bits: int = 12) -> int:
    return int(format(i, "0%db" % bits)[::-1], 2)


ROOTS = [pow(OMEGA, brp(i), R) for i in range(N)]


def hash_to_bls_field(b: bytes) -> int:
    return int.from_bytes(hashlib.sha256(b).digest(), "big") % R


def bytes_to_bls_field(b: bytes) -> int:
    v = int.from_bytes(b, "big")
    if len(b) != 32 or v >= R:
        raise ValueError("not a canonical field element")
    return v


def fe(v: int) -> bytes:
    return (v % R).to_bytes(32, "big")


def blob_from_ints(vals) -> bytes:
    assert len(vals) == N
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def blob_to_ints(blob: bytes):
    assert len(blob) == BYTES_PER_BLOB
    return [bytes_to_bls_field(blob[32 * i:32 * i + 32]) for i in range(N)]


def transcript(blob: bytes, commitment: bytes) -> bytes:
    return FS_DOMAIN + N.to_bytes(16, "big") + blob + commitment


def compute_challenge(blob: bytes, commitment: bytes) -> int:
    return hash_to_bls_field(transcript(blob, commitment))


def _batch_inverse(vals):
    pre, acc = [], 1
    for v in vals:
        acc = acc * v % R
        pre.append(acc)
    inv = pow(acc, -1, R)
    out = [0] * len(vals)
    for k in range(len(vals) - 1, -1, -1):
        out[k] = inv * (pre[k - 1] if k else 1) % R
        inv = inv * vals[k] % R
    return out


def evaluate(f, z: int) -> int:
    """evaluate_polynomial_in_evaluation_form: f in brp order over ROOTS."""
    z %= R
    for i, w in enumerate(ROOTS):
        if w == z:
            return f[i] % R
    inv = _batch_inverse([(z - w) % R for w in ROOTS])
    s = sum(fi * w % R * iv for fi, w, iv in zip(f, ROOTS, inv)) % R
    return (pow(z, N, R) - 1) * pow(N, -1, R) % R * s % R


def validate_kzg_g1(b: bytes):
    """-> affine point or None (infinity); raises on anything c-kzg refuses."""
    if len(b) != 48:
        raise ValueError("length")
    if b == G1_INF:
        return None
    if not b[0] & 0x80:
        raise ValueError("not compressed")
    pt = O.g1_from_bytes(b)
    if pt is None or not O.g1_in_subgroup(pt):
        raise ValueError("not in G1")
    return pt


def rho_powers(commitments, zs, ys, proofs):
    n = len(commitments)
    data = RC_DOMAIN + N.to_bytes(8, "big") + n.to_bytes(8, "big")
    for c, z, y, p in zip(commitments, zs, ys, proofs):
        data += c + fe(z) + fe(y) + p
    rho = hash_to_bls_field(data)
    return [pow(rho, i, R) for i in range(n)]


def pairing_check(a, b, tau_g2) -> bool:
    """e(A, -[tau]_2) e(B, G2) == 1; a pair whose G1 side is infinity contributes 1."""
    f = None
    for p, q in ((a, O.E2.neg(tau_g2)), (b, O.G2)):
        if p is None:
            continue
        m = O.miller_loop(p, q)
        f = m if f is None else O.f12_mul(f, m)
    return True if f is None else O.f12_is_one(O.final_exp(f))


def verify_kzg_proof_batch(commitments, zs, ys, proofs, tau_g2, weights=None) -> bool:
    """The spec's batch check with the oracle's pairing (about a second)."""
    cs = [validate_kzg_g1(c) for c in commitments]
    ps = [validate_kzg_g1(p) for p in proofs]
    w = weights if weights is not None else rho_powers(commitments, zs, ys, proofs)
    a = b = None
    for c, z, y, p, wi in zip(cs, zs, ys, ps, w):
        a = O.g1_add(a, O.g1_mul(p, wi))
        t = O.g1_add(c, O.g1_mul(O.G1, (-y) % R))
        b = O.g1_add(b, O.g1_mul(t, wi))
        b = O.g1_add(b, O.g1_mul(p, wi * z % R))
    return pairing_check(a, b, tau_g2)


def verify_blob_kzg_proof_batch(blobs, commitments, proofs, tau_g2) -> bool:
    zs = [compute_challenge(b, c) for b, c in zip(blobs, commitments)]
    ys = [evaluate(blob_to_ints(b), z) for b, z in zip(blobs, zs)]
    return verify_kzg_proof_batch(commitments, zs, ys, proofs, tau_g2)


class TestSetup:
    """A trusted setup whose secret is known: not secure, exact by construction."""
    __test__ = False

    def __init__(self, tau: int = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF % R):
        self.tau = tau
        assert tau not in ROOTS
        self.tau_g2_point = O.g2_mul(O.G2, tau)
        self.tau_g2 = O.g2_to_bytes(self.tau_g2_point)

    def at_tau(self, f) -> int:
        return evaluate(f, self.tau)

    def commit(self, f) -> bytes:
        return O.g1_to_bytes(O.g1_mul(O.G1, self.at_tau(f)))

    def proof(self, f, z: int, y: int = None, extra: int = 0) -> bytes:
        """[(f(tau) - y) / (tau - z) + extra]G1 (y defaults to f(z))."""
        y = evaluate(f, z) if y is None else y
        q = (self.at_tau(f) - y) * pow(self.tau - z, -1, R) + extra
        return O.g1_to_bytes(O.g1_mul(O.G1, q % R))

    def blob_case(self, f):
        """-> (blob, commitment, proof, z, y) of an honest sidecar for the polynomial f."""
        blob = blob_from_ints(f)
        c = self.commit(f)
        z = compute_challenge(blob, c)
        y = evaluate(f, z)
        return blob, c, self.proof(f, z, y), z, y


def random_poly(seed: int):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(N)]


def kat_poly():
    """The golden KAT's blob recipe: element i = SHA-256("kzg-kat" | LE32(i)) mod r."""
    return [hash_to_bls_field(b"kzg-kat" + i.to_bytes(4, "little")) for i in range(N)]
