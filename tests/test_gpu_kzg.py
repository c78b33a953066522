"""Blob KZG proof verification on the GPU (lb_kzg_*, lodestar_amd/csrc/k_kzg.hip) against
the Python restatement in tests/kzg_helper.py.  Every comparison is exact.  The trusted
setup is a test setup with a known tau, so a commitment or proof is one scalar
multiplication and every expected verdict is known by construction; the mainnet KAT
(tests/golden/kzg_mainnet_kat.json) ties the same code to the ceremony's [tau]_2."""
import functools
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from lodestar_amd import kzg, native
from lodestar_amd.native import Device, LodestarBlsError, pack_blobs
from oracle import bls12_381 as O
from tests import g1_edges_helper as H
from tests import kzg_helper as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, N = K.R, K.N
S = K.TestSetup()
OK, BAD_BLOB, BAD_COMMITMENT, BAD_PROOF, BAD_SCALAR = range(5)


@functools.lru_cache(None)
def cases():
    """Nine honest sidecars (blob, commitment, proof, z, y) with their polynomials."""
    out = []
    for i in range(9):
        f = K.random_poly(100 + i)
        out.append((f,) + S.blob_case(f))
    return out


def columns(cs):
    return [c[1] for c in cs], [c[2] for c in cs], [c[3] for c in cs]


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(autouse=True)
def test_setup_loaded(dev):
    dev.kzg_load_setup(S.tau_g2)


# ---- evaluation ------------------------------------------------------------------------
def eval_blobs():
    single = [0] * N
    single[N - 1] = 12345
    return [[0] * N, [77] * N, [R - 1] * N, K.random_poly(5), single]


def test_evaluate_matches_the_barycentric_formula(dev):
    zs = [K.ROOTS[0], K.ROOTS[1], K.ROOTS[N - 1], 0, 2, R - 1, 0x1CE1CE1CE % R * 0xABCDEF123456789 % R]
    polys = eval_blobs()
    pairs = [(f, z) for f in polys for z in zs]
    ys, st = dev.kzg_evaluate([K.blob_from_ints(f) for f, _ in pairs], [K.fe(z) for _, z in pairs])
    assert st == [OK] * len(pairs)
    assert ys == [K.fe(K.evaluate(f, z)) for f, z in pairs]
    # the equality branch returns that element
    f = polys[3]
    assert ys[3 * len(zs)] == K.fe(f[0]) and ys[3 * len(zs) + 1] == K.fe(f[1]) and ys[3 * len(zs) + 2] == K.fe(f[N - 1])


def test_evaluate_statuses(dev):
    f = K.random_poly(6)
    good = K.blob_from_ints(f)
    first = R.to_bytes(32, "big") + good[32:]
    last = good[:-32] + R.to_bytes(32, "big")
    blobs = [good, good, good, first, last, good]
    zs = [K.fe(5), R.to_bytes(32, "big"), (2 ** 256 - 1).to_bytes(32, "big"), K.fe(5), K.fe(5), K.fe(R - 1)]
    ys, st = dev.kzg_evaluate(blobs, zs)
    assert st == [OK, BAD_SCALAR, BAD_SCALAR, BAD_BLOB, BAD_BLOB, OK]
    assert ys[0] == K.fe(K.evaluate(f, 5)) and ys[5] == K.fe(K.evaluate(f, R - 1))
    assert ys[1:5] == [bytes(32)] * 4


# ---- challenges ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 9])
def test_blob_challenges(dev, n):
    cs = cases()[:n]
    blobs, coms, _ = columns(cs)
    zs, ys, st = dev.kzg_blob_challenges(blobs, coms)
    assert st == [OK] * n
    for (f, blob, c, _, z, y), zg, yg in zip(cs, zs, ys):
        digest = hashlib.sha256(K.FS_DOMAIN + N.to_bytes(16, "big") + blob + c).digest()
        assert zg == (int.from_bytes(digest, "big") % R).to_bytes(32, "big") == K.fe(z)
        assert yg == K.fe(y)


def test_blob_challenges_flag_a_bad_blob(dev):
    _, blob, c, _, _, _ = cases()[0]
    bad = blob[:32 * 2047] + (R + 1).to_bytes(32, "big") + blob[32 * 2048:]
    zs, ys, st = dev.kzg_blob_challenges([blob, bad], [c, c])
    assert st == [OK, BAD_BLOB] and zs[1] == bytes(32) and ys[1] == bytes(32)


# ---- verdicts --------------------------------------------------------------------------
def test_empty_batch_is_true(dev):
    assert dev.kzg_verify_blob_proof_batch([], [], [], each=True) == (True, [], [])
    assert dev.kzg_verify_proof_batch([], [], [], []) == (True, [])


@pytest.mark.parametrize("n", [1, 2, 6, 9])
def test_honest_batches(dev, n):
    blobs, coms, proofs = columns(cases()[:n])
    assert dev.kzg_verify_blob_proof_batch(blobs, coms, proofs, each=True) == (True, [OK] * n, [1] * n)
    assert dev.kzg_verify_blob_proof_batch(blobs, coms, proofs) == (True, [OK] * n)


def test_a_foreign_proof_fails_and_is_named(dev):
    blobs, coms, proofs = columns(cases()[:6])
    proofs[2] = proofs[3]
    assert dev.kzg_verify_blob_proof_batch(blobs, coms, proofs, each=True) == (False, [OK] * 6, [1, 1, 0, 1, 1, 1])
    assert dev.kzg_verify_blob_proof_batch(blobs, coms, proofs) == (False, [OK] * 6)


def test_swapped_commitments_fail(dev):
    blobs, coms, proofs = columns(cases()[:3])
    coms[0], coms[1] = coms[1], coms[0]
    assert dev.kzg_verify_blob_proof_batch(blobs, coms, proofs, each=True) == (False, [OK] * 3, [0, 0, 1])


def test_infinity_proofs_and_commitments(dev):
    const = [31337] * N
    blob_c, com_c, proof_c, _, _ = S.blob_case(const)
    assert proof_c == K.G1_INF and com_c != K.G1_INF
    blob_0, com_0, proof_0, _, _ = S.blob_case([0] * N)
    assert proof_0 == K.G1_INF and com_0 == K.G1_INF
    assert dev.kzg_verify_blob_proof_batch([blob_c], [com_c], [proof_c], each=True) == (True, [OK], [1])
    assert dev.kzg_verify_blob_proof_batch([blob_0], [com_0], [proof_0], each=True) == (True, [OK], [1])
    assert dev.kzg_verify_blob_proof_batch([blob_0, blob_c], [com_0, com_c], [proof_0, proof_c],
                                           each=True) == (True, [OK] * 2, [1, 1])
    # a constant blob under the zero blob's (infinite) commitment is a failed check, not an error
    assert dev.kzg_verify_blob_proof_batch([blob_c], [com_0], [proof_c], each=True) == (False, [OK], [0])


def test_cancelling_pair_needs_the_rho_powers(dev):
    """pi_0 + [d/(tau - z_0)]G1 and pi_1 - [d/(tau - z_1)]G1: the errors cancel in the unweighted
    sum (asserted with the oracle's pairing), so only the powers of rho reject the batch."""
    (f0, b0, c0, _, z0, y0), (f1, b1, c1, _, z1, y1) = cases()[:2]
    d = 0xD15EA5E
    p0 = S.proof(f0, z0, y0, extra=d * pow(S.tau - z0, -1, R))
    p1 = S.proof(f1, z1, y1, extra=-d * pow(S.tau - z1, -1, R))
    assert K.verify_kzg_proof_batch([c0, c1], [z0, z1], [y0, y1], [p0, p1], S.tau_g2_point, weights=[1, 1]) is True
    assert dev.kzg_verify_blob_proof_batch([b0, b1], [c0, c1], [p0, p1], each=True) == (False, [OK, OK], [0, 0])


# ---- encodings -------------------------------------------------------------------------
def test_bad_encodings_are_statuses_not_verdicts(dev):
    blobs, coms, proofs = columns(cases()[:4])
    outside = O.g1_to_bytes(O.g1_add(O.g1_from_bytes(coms[1]), H.torsion_point()))
    assert not O.g1_in_subgroup(O.g1_from_bytes(outside))
    c2 = list(coms)
    c2[1] = outside
    assert dev.kzg_verify_blob_proof_batch(blobs, c2, proofs, each=True) == (
        False, [OK, BAD_COMMITMENT, OK, OK], [1, 0, 1, 1])
    p2 = list(proofs)
    p2[3] = bytes([proofs[3][0] & 0x7F]) + proofs[3][1:]
    assert dev.kzg_verify_blob_proof_batch(blobs, coms, p2, each=True) == (False, [OK, OK, OK, BAD_PROOF], [1, 1, 1, 0])
    p3 = list(proofs)
    xp = bytearray((O.P + 5).to_bytes(48, "big"))
    xp[0] |= 0x80
    p3[0] = bytes(xp)
    assert dev.kzg_verify_blob_proof_batch(blobs, coms, p3) == (False, [BAD_PROOF, OK, OK, OK])
    bad_blob = R.to_bytes(32, "big") + blobs[2][32:]
    assert dev.kzg_verify_blob_proof_batch(blobs[:2] + [bad_blob], coms[:3], proofs[:3]) == (
        False, [OK, OK, BAD_BLOB])


# ---- point evaluation ------------------------------------------------------------------
def test_verify_proof_batch(dev):
    cs = cases()[:3]
    coms, proofs = [c[2] for c in cs], [c[3] for c in cs]
    zs, ys = [K.fe(c[4]) for c in cs], [K.fe(c[5]) for c in cs]
    assert dev.kzg_verify_proof_batch(coms, zs, ys, proofs, each=True) == (True, [OK] * 3, [1] * 3)
    wrong = list(ys)
    wrong[1] = K.fe(cs[1][5] + 1)
    assert dev.kzg_verify_proof_batch(coms, zs, wrong, proofs, each=True) == (False, [OK] * 3, [1, 0, 1])
    big = list(ys)
    big[2] = R.to_bytes(32, "big")
    assert dev.kzg_verify_proof_batch(coms, zs, big, proofs, each=True) == (False, [OK, OK, BAD_SCALAR], [1, 1, 0])
    bigz = list(zs)
    bigz[0] = (2 ** 256 - 1).to_bytes(32, "big")
    assert dev.kzg_verify_proof_batch(coms, bigz, ys, proofs) == (False, [BAD_SCALAR, OK, OK])


# ---- setup -----------------------------------------------------------------------------
def test_verify_before_load_is_an_error():
    d = Device(0)
    try:
        assert d.kzg_setup_loaded() is False
        blobs, coms, proofs = columns(cases()[:1])
        with pytest.raises(LodestarBlsError, match="no trusted setup"):
            d.kzg_verify_blob_proof_batch(blobs, coms, proofs)
        d.kzg_load_setup(S.tau_g2)
        assert d.kzg_setup_loaded() is True
        assert d.kzg_verify_blob_proof_batch(blobs, coms, proofs) == (True, [OK])
    finally:
        d.close()


def twist_point_outside_g2():
    x = (3, 1)
    while True:
        y = O.f2_sqrt(O.f2_add(O.f2_mul(O.f2_sqr(x), x), (4, 4)))
        if y is not None and not O.g2_in_subgroup((x, y)):
            return O.g2_to_bytes((x, y))
        x = (x[0] + 1, 1)


def test_a_refused_setup_keeps_the_old_one(dev):
    blobs, coms, proofs = columns(cases()[:2])
    for bad, why in ((b"\xc0" + bytes(95), "infinity"), (twist_point_outside_g2(), "not in G2"),
                     (bytes(96), "does not decode")):
        with pytest.raises(LodestarBlsError, match=why):
            dev.kzg_load_setup(bad)
        assert dev.kzg_setup_loaded() is True
        assert dev.kzg_verify_blob_proof_batch(blobs, coms, proofs) == (True, [OK] * 2)


def test_mainnet_kat(dev):
    with open(os.path.join(ROOT, "tests", "golden", "kzg_mainnet_kat.json")) as f:
        kat = json.load(f)
    blob = K.blob_from_ints(K.kat_poly())
    c, p = bytes.fromhex(kat["commitment"]), bytes.fromhex(kat["proof"])
    dev.kzg_load_setup(bytes.fromhex(kat["g2_tau"]))
    zs, ys, st = dev.kzg_blob_challenges([blob], [c])
    assert (zs[0].hex(), ys[0].hex(), st) == (kat["z"], kat["y"], [OK])
    assert dev.kzg_verify_blob_proof_batch([blob], [c], [p], each=True) == (True, [OK], [1])
    assert dev.kzg_verify_proof_batch([c], zs, ys, [p]) == (True, [OK])
    dev.kzg_load_setup(S.tau_g2)
    assert dev.kzg_verify_blob_proof_batch([blob], [c], [p], each=True) == (False, [OK], [0])


# ---- size limit and interference -------------------------------------------------------
def test_more_than_the_maximum_is_refused(dev):
    n = native.LB_KZG_MAX_BLOBS + 1
    with pytest.raises(LodestarBlsError, match="LB_KZG_MAX_BLOBS"):
        dev.kzg_verify_blob_proof_batch([bytes(K.BYTES_PER_BLOB)] * n, [K.G1_INF] * n, [K.G1_INF] * n)


def test_a_kzg_verify_between_signature_calls_leaves_them_alone(dev):
    sks = [O.interop_secret_key(i) for i in range(4)]
    msgs = [hashlib.sha256(b"kzg-between" + bytes([i])).digest() for i in range(4)]
    msgs_bad = msgs[:3] + [bytes(32)]
    sk_be = [sk.to_bytes(32, "big") for sk in sks]
    pks, sigs = dev.sk_to_pk(sk_be), dev.sign(sk_be, msgs)
    blob, offs = pack_blobs(sigs)

    def signatures():
        res = dev.verify_requests(np.array([0, 3, 4], np.uint32), np.frombuffer(b"".join(pks), np.uint8), None,
                                  np.frombuffer(b"".join(msgs_bad), np.uint8), blob, offs, bytes(32))
        return [bool(v) for v in res.valid]

    dev.pubkey_table_append(pks[:2])
    before = signatures()
    blobs, coms, proofs = columns(cases()[:6])
    assert dev.kzg_verify_blob_proof_batch(blobs, coms, proofs) == (True, [OK] * 6)
    assert signatures() == before == [True, False]
    assert dev.pubkey_table_read(0, 2) == pks[:2]
    assert [n for n, _ in dev.last_stage_times()] != ["kzg_hash", "kzg_eval", "kzg_tail"]
    dev.kzg_verify_blob_proof_batch(blobs[:1], coms[:1], proofs[:1])
    assert [n for n, _ in dev.last_stage_times()] == ["kzg_hash", "kzg_eval", "kzg_tail"]


# ---- through the hosts -------------------------------------------------------------------
def write_test_setup(tmp_path):
    g1 = [K.G1_INF.hex()] * 4096
    g2 = [O.g2_to_bytes(O.G2).hex(), S.tau_g2.hex()] + [O.g2_to_bytes(O.G2).hex()] * 63
    path = tmp_path / "trusted_setup.txt"
    path.write_text("4096\n65\n" + "\n".join(g1 + g2) + "\n")
    return path


def test_js_kzg_object_through_the_addon(tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "lodestar_amd", "napi", "lodestar_bls.node")
    if node is None or not os.path.exists(addon):
        pytest.skip("node or the addon not present")
    write_test_setup(tmp_path)
    blobs, coms, proofs = columns(cases()[:3])
    for name, items in (("blobs", blobs), ("commitments", coms), ("proofs", proofs)):
        (tmp_path / (name + ".bin")).write_bytes(b"".join(items))
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "kzg_gpu.js"), str(tmp_path)], capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "kzg gpu ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_gpu_kzg_raises_or_returns_false(dev, tmp_path):
    path = write_test_setup(tmp_path)
    g = kzg.GpuKzg(dev)
    g.load_trusted_setup(str(path))
    blobs, coms, proofs = columns(cases()[:3])
    assert g.verify_blob_kzg_proof_batch(blobs, coms, proofs) is True
    assert g.verify_blob_kzg_proof(blobs[0], coms[0], proofs[0]) is True
    assert g.verify_blob_kzg_proof(blobs[0], coms[0], proofs[1]) is False
    assert g.verify_blob_kzg_proof_batch(blobs, coms, [proofs[1], proofs[0], proofs[2]]) is False
    assert g.verify_blob_kzg_proof_batch([], [], []) is True
    with pytest.raises(kzg.KzgError, match="BAD_BLOB"):
        g.verify_blob_kzg_proof(R.to_bytes(32, "big") + blobs[0][32:], coms[0], proofs[0])
    with pytest.raises(kzg.KzgError, match="BAD_PROOF"):
        g.verify_blob_kzg_proof(blobs[0], coms[0], bytes(48))
    with pytest.raises(kzg.KzgError):
        g.verify_blob_kzg_proof_batch(blobs, coms, proofs[:2])
