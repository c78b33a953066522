"""Blob KZG commitments and proofs restated on Python integers, on top of tests/kzg_helper.py:
the Lagrange scalars of a setup whose tau is known, the MSM's signed digits, and the quotient
polynomial of compute_kzg_proof_impl (both branches).  No c-kzg source or vector is involved.
"""
from __future__ import annotations

from oracle import bls12_381 as O
from tests import kzg_helper as K

R, N = K.R, K.N


def lagrange_scalars(tau: int):
    """l_i = L_i(tau) = w_i (tau^N - 1) / (N (tau - w_i)), spec (brp) order: KZG_SETUP_G1_LAGRANGE[i] = [l_i]G1."""
    inv = K._batch_inverse([N * (tau - w) % R for w in K.ROOTS])
    t = (pow(tau, N, R) - 1) % R
    return [w * t % R * iv % R for w, iv in zip(K.ROOTS, inv)]


def recode(v: int):
    """32 signed base-256 digits in [-127, 128], least significant first; v < r."""
    out, carry = [], 0
    for j in range(32):
        raw = ((v >> (8 * j)) & 0xFF) + carry
        if raw > 128:
            out.append(raw - 256)
            carry = 1
        else:
            out.append(raw)
            carry = 0
    assert carry == 0
    return out


def quotient(f, z: int):
    """-> (q, y): compute_kzg_proof_impl's quotient in evaluation form and y = f(z)."""
    z %= R
    y = K.evaluate(f, z)
    m = K.ROOTS.index(z) if z in K.ROOTS else None
    inv = _inverse_skipping([(w - z) % R for w in K.ROOTS], m)
    q = [(fi - y) * iv % R for fi, iv in zip(f, inv)]
    if m is not None:
        # compute_quotient_eval_within_domain: sum_(i != m) (f_i - y) w_i / (z (z - w_i))
        zi = _inverse_skipping([z * (z - w) % R for w in K.ROOTS], m)
        q[m] = sum((f[i] - y) * K.ROOTS[i] % R * zi[i] for i in range(N) if i != m) % R
    return q, y


def _inverse_skipping(vals, skip):
    vals = list(vals)
    if skip is not None:
        vals[skip] = 1
    out = K._batch_inverse(vals)
    if skip is not None:
        out[skip] = 0
    return out


def file_order(xs):
    """Spec-order items -> the order of trusted_setup.txt: file[brp(i)] = spec[i]."""
    out = [None] * len(xs)
    for i, x in enumerate(xs):
        out[K.brp(i)] = x
    return out


def g1_compress(pk96: bytes) -> bytes:
    """96-byte uncompressed affine G1 (or 0x40 00...) -> the 48-byte compressed form."""
    assert len(pk96) == 96
    if pk96[0] & 0x40:
        return K.G1_INF
    y = int.from_bytes(pk96[48:], "big")
    return bytes([pk96[0] | 0x80 | (0x20 if y > (O.P - 1) // 2 else 0)]) + pk96[1:48]


def scalars_blob(vals) -> bytes:
    """4096 scalars -> one lincomb job (big-endian, 32 bytes each; values are written as given)."""
    assert len(vals) == N
    return b"".join(int(v).to_bytes(32, "big") for v in vals)


def setup_text(g1_file_order, tau_g2: bytes) -> str:
    g2 = [O.g2_to_bytes(O.G2).hex(), tau_g2.hex()] + [O.g2_to_bytes(O.G2).hex()] * 63
    return "4096\n65\n" + "\n".join([p.hex() for p in g1_file_order] + g2) + "\n"
