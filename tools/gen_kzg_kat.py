"""Regenerate tests/golden/kzg_mainnet_kat.json from a ceremony ``trusted_setup.txt``.

Usage: python tools/gen_kzg_kat.py path/to/trusted_setup.txt [out.json]

The file lists the 4096 Lagrange G1 points in natural order (the spec's KZG_SETUP_G1_LAGRANGE
is their bit-reversal permutation: L[brp(i)]) and the 65 monomial G2 points.  The KAT is one
blob given as a recipe (tests/kzg_helper.kat_poly: the 128 KiB are not stored), its commitment
sum f_i L_i and the proof sum q_i L_i of the quotient q_i = (f_i - y) / (w_i - z) at the blob's
own challenge z -- two 4096-term sums in pure Python (about a minute) -- checked here with the
oracle's pairing: e(proof, [tau - z]_2) == e(C - [y]G1, G2).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import bls12_381 as O  # noqa: E402
from tests import kzg_helper as K  # noqa: E402


def lincomb(points, scalars):
    acc = None
    for p, s in zip(points, scalars):
        acc = O.g1_add(acc, O.g1_mul(p, s % K.R))
    return acc


def main():
    src = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "kzg_mainnet_kat.json")
    lines = open(src).read().split()
    n1, n2 = int(lines[0]), int(lines[1])
    assert (n1, n2) == (K.N, 65)
    g1 = [O.g1_from_bytes(bytes.fromhex(x)) for x in lines[2:2 + n1]]
    g2 = lines[2 + n1:2 + n1 + n2]
    assert bytes.fromhex(g2[0]) == O.g2_to_bytes(O.G2)
    lagrange = [g1[K.brp(i)] for i in range(K.N)]  # spec order
    tau_g2 = O.g2_from_bytes(bytes.fromhex(g2[1]))
    f = K.kat_poly()
    blob = K.blob_from_ints(f)
    c_pt = lincomb(lagrange, f)
    c = O.g1_to_bytes(c_pt)
    z = K.compute_challenge(blob, c)
    y = K.evaluate(f, z)
    assert z not in K.ROOTS
    q = [(fi - y) * pow(w - z, -1, K.R) % K.R for fi, w in zip(f, K.ROOTS)]
    p_pt = lincomb(lagrange, q)
    p = O.g1_to_bytes(p_pt)
    # e(proof, [tau]_2 - [z]G2) == e(C - [y]G1, G2)
    lhs = O.pairing(p_pt, O.g2_add(tau_g2, O.g2_mul(O.G2, (-z) % K.R)))
    rhs = O.pairing(O.g1_add(c_pt, O.g1_mul(O.G1, (-y) % K.R)), O.G2)
    assert O.f12_eq(lhs, rhs), "the generated proof does not verify"
    doc = {
        "source": "KZG ceremony trusted_setup.txt: G2 monomial point 1, and one blob proved with its Lagrange points",
        "g2_tau": g2[1],
        "blob_recipe": 'element i = SHA-256("kzg-kat" | LE32(i)) mod r, i = 0..4095',
        "commitment": c.hex(),
        "proof": p.hex(),
        "z": K.fe(z).hex(),
        "y": K.fe(y).hex(),
    }
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
