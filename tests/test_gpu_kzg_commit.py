"""Blob KZG commitments and proofs on the GPU (lb_kzg_blob_commitments / _blob_proofs /
_compute_proofs / _g1_lincomb, lodestar_amd/csrc/k_kzg_msm.hip) against the restatement in
tests/kzg_helper.py and tests/kzg_commit_helper.py.  Every comparison is exact (bytes).

Setup A is an honest Lagrange setup of a known tau, so a commitment is [f(tau)]G1 and a proof
[(f(tau) - y) / (tau - z)]G1: one oracle multiplication each.  Setup B is built for the MSM's
digit and group-law edges: equal, opposite and [256]-related points and three at infinity.
The points of both are made on the GPU (sk_to_pk) and spot-checked against the oracle."""
import functools
import hashlib
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from lodestar_amd import kzg, native
from lodestar_amd.native import Device, LodestarBlsError, pack_blobs
from oracle import bls12_381 as O
from tests import g1_edges_helper as H
from tests import kzg_commit_helper as C
from tests import kzg_helper as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, N = K.R, K.N
S = K.TestSetup()
OK, BAD_BLOB, BAD_COMMITMENT, BAD_PROOF, BAD_SCALAR = range(5)
INF = K.G1_INF


def g1_of(scalar: int) -> bytes:
    return O.g1_to_bytes(O.g1_mul(O.G1, scalar % R)) if scalar % R else INF


def points_of(dev, scalars):
    """[s]G1 compressed, on the GPU; infinity for s = 0."""
    pks = dev.sk_to_pk([(s if s else 1).to_bytes(32, "big") for s in scalars])
    return [C.g1_compress(p) if s else INF for p, s in zip(pks, scalars)]


@pytest.fixture(scope="module")
def dev():
    d = Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def setup_a(dev):
    """The honest setup's G1 lines, in file order."""
    lag = C.lagrange_scalars(S.tau)
    pts = points_of(dev, lag)
    for i in (0, 1, 2047, N - 1):
        assert pts[i] == g1_of(lag[i])
    return b"".join(C.file_order(pts))


B_A0, B_DELTA = 0x1F2E3D4C5B6A79880123456789ABCDEF % R, 0x0123456789ABCDEFFEDCBA9876543210F % R


@functools.lru_cache(None)
def b_scalars():
    a = [(B_A0 + i * B_DELTA) % R for i in range(N)]
    a[1] = a[0]
    a[2] = R - a[0]
    a[3] = 256 * a[0] % R
    a[4] = pow(2, 248, R) * a[0] % R
    a[5] = a[6] = a[7] = 0
    return a


@pytest.fixture(scope="module")
def setup_b(dev):
    a = b_scalars()
    pts = points_of(dev, a)
    for i in (0, 2, 4, 5, N - 1):
        assert pts[i] == g1_of(a[i])
    return b"".join(C.file_order(pts))


@pytest.fixture(autouse=True)
def honest_setup_loaded(dev, setup_a):
    dev.kzg_load_setup(S.tau_g2)
    dev.kzg_load_setup_g1(setup_a)


@functools.lru_cache(None)
def cases():
    """The nine honest sidecars of tests/test_gpu_kzg.py's recipe: (f, blob, commitment, proof, z, y)."""
    out = []
    for i in range(9):
        f = K.random_poly(100 + i)
        out.append((f,) + S.blob_case(f))
    return out


# ---- commitments and blob proofs -------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 9])
def test_commitments_and_blob_proofs_are_the_honest_ones(dev, n):
    cs = cases()[:n]
    blobs = [c[1] for c in cs]
    coms, st = dev.kzg_blob_commitments(blobs)
    assert st == [OK] * n and coms == [c[2] for c in cs]
    proofs, st = dev.kzg_blob_proofs(blobs, coms)
    assert st == [OK] * n and proofs == [c[3] for c in cs]
    assert dev.kzg_verify_blob_proof_batch(blobs, coms, proofs, each=True) == (True, [OK] * n, [1] * n)


def test_one_more_blob_than_a_group(dev):
    """A call runs its MSMs in groups of 16 jobs: 17 blobs cross into a second group."""
    n = 17
    polys = [[(1000 * k + i) % 65537 for i in range(N)] for k in range(n)]
    coms, st = dev.kzg_blob_commitments([K.blob_from_ints(f) for f in polys])
    assert st == [OK] * n and coms == [S.commit(f) for f in polys]


def test_compute_proofs_outside_and_inside_the_domain(dev):
    f = cases()[0][0]
    blob = cases()[0][1]
    zs = [2, R - 1, 0x1CE1CE1CE % R * 0xABCDEF123456789 % R, K.ROOTS[0], K.ROOTS[1], K.ROOTS[N - 1]]
    proofs, ys, st = dev.kzg_compute_proofs([blob] * len(zs), [K.fe(z) for z in zs])
    assert st == [OK] * len(zs)
    for z, p, y in zip(zs, proofs, ys):
        yy = K.evaluate(f, z)
        assert y == K.fe(yy) and p == S.proof(f, z, yy)
    assert ys[3:] == [K.fe(f[0]), K.fe(f[1]), K.fe(f[N - 1])]
    assert dev.kzg_verify_proof_batch([cases()[0][2]] * len(zs), [K.fe(z) for z in zs], ys, proofs,
                                      each=True) == (True, [OK] * len(zs), [1] * len(zs))


def test_edge_polynomials(dev):
    single = [0] * N
    single[N - 1] = 12345
    polys = [[0] * N, [31337] * N, [R - 1] * N, single]
    blobs = [K.blob_from_ints(f) for f in polys]
    coms, st = dev.kzg_blob_commitments(blobs)
    assert st == [OK] * 4 and coms == [S.commit(f) for f in polys]
    assert coms[0] == INF and coms[1] != INF
    proofs, st = dev.kzg_blob_proofs(blobs, coms)
    assert st == [OK] * 4 and proofs == [S.blob_case(f)[2] for f in polys]
    assert proofs[0] == INF and proofs[1] == INF and proofs[3] != INF
    assert dev.kzg_verify_blob_proof_batch(blobs, coms, proofs, each=True) == (True, [OK] * 4, [1] * 4)


def test_statuses_zero_the_item_and_spare_its_neighbours(dev):
    f, blob, com, proof, _, _ = cases()[0]
    first = R.to_bytes(32, "big") + blob[32:]
    last = blob[:-32] + R.to_bytes(32, "big")
    coms, st = dev.kzg_blob_commitments([first, blob, last])
    assert st == [BAD_BLOB, OK, BAD_BLOB] and coms == [bytes(48), com, bytes(48)]
    outside = O.g1_to_bytes(O.g1_add(O.g1_from_bytes(com), H.torsion_point()))
    assert not O.g1_in_subgroup(O.g1_from_bytes(outside))
    cleared = bytes([com[0] & 0x7F]) + com[1:]
    proofs, st = dev.kzg_blob_proofs([blob, blob, blob, first, last], [outside, com, cleared, com, com])
    assert st == [BAD_COMMITMENT, OK, BAD_COMMITMENT, BAD_BLOB, BAD_BLOB]
    assert proofs == [bytes(48), proof, bytes(48), bytes(48), bytes(48)]
    zs = [R.to_bytes(32, "big"), K.fe(5), (2 ** 256 - 1).to_bytes(32, "big"), K.fe(5)]
    proofs, ys, st = dev.kzg_compute_proofs([blob, blob, blob, last], zs)
    assert st == [BAD_SCALAR, OK, BAD_SCALAR, BAD_BLOB]
    y5 = K.evaluate(f, 5)
    assert proofs == [bytes(48), S.proof(f, 5, y5), bytes(48), bytes(48)]
    assert ys == [bytes(32), K.fe(y5), bytes(32), bytes(32)]


def test_a_foreign_commitment_is_hashed_not_compared(dev):
    (f0, b0, c0, p0, _, _), (_, _, c1, _, _, _) = cases()[:2]
    proofs, st = dev.kzg_blob_proofs([b0], [c1])
    z = K.compute_challenge(b0, c1)
    assert st == [OK] and proofs[0] != p0 and proofs[0] == S.proof(f0, z)


def test_sizes_and_null_setup(dev):
    n = native.LB_KZG_MAX_BLOBS + 1
    with pytest.raises(LodestarBlsError, match="LB_KZG_MAX_BLOBS"):
        dev.kzg_blob_commitments([bytes(K.BYTES_PER_BLOB)] * n)
    assert dev.kzg_blob_commitments([]) == ([], [])
    assert dev.kzg_blob_proofs([], []) == ([], [])


def test_a_proof_call_before_any_g1_load_is_an_error():
    d = Device(0)
    try:
        assert d.kzg_setup_g1_loaded() is False
        _, blob, com, proof, _, _ = cases()[0]
        for call in (lambda: d.kzg_blob_proofs([blob], [com]), lambda: d.kzg_blob_commitments([blob]),
                     lambda: d.kzg_compute_proofs([blob], [K.fe(2)]), lambda: d.kzg_g1_lincomb([blob])):
            with pytest.raises(LodestarBlsError, match="no G1 setup"):
                call()
        d.kzg_load_setup(S.tau_g2)
        assert d.kzg_setup_loaded() is True and d.kzg_setup_g1_loaded() is False
        assert d.kzg_verify_blob_proof_batch([blob], [com], [proof]) == (True, [OK])
    finally:
        d.close()


def test_a_commit_call_between_signature_calls_leaves_them_alone(dev):
    sks = [O.interop_secret_key(i) for i in range(4)]
    msgs = [hashlib.sha256(b"kzg-commit-between" + bytes([i])).digest() for i in range(4)]
    msgs_bad = msgs[:3] + [bytes(32)]
    sk_be = [sk.to_bytes(32, "big") for sk in sks]
    pks, sigs = dev.sk_to_pk(sk_be), dev.sign(sk_be, msgs)
    blob, offs = pack_blobs(sigs)

    def signatures():
        res = dev.verify_requests(np.array([0, 3, 4], np.uint32), np.frombuffer(b"".join(pks), np.uint8), None,
                                  np.frombuffer(b"".join(msgs_bad), np.uint8), blob, offs, bytes(32))
        return [bool(v) for v in res.valid]

    size = dev.pubkey_table_size()
    dev.pubkey_table_append(pks[:2])
    before = signatures()
    cs = cases()[:2]
    blobs = [c[1] for c in cs]
    coms, st = dev.kzg_blob_commitments(blobs)
    assert st == [OK, OK] and coms == [c[2] for c in cs]
    assert [n for n, _ in dev.last_stage_times()] == ["kzg_msm"]
    assert signatures() == before == [True, False]
    assert dev.pubkey_table_read(size, 2) == pks[:2]
    proofs, st = dev.kzg_blob_proofs(blobs, coms)
    assert [n for n, _ in dev.last_stage_times()] == ["kzg_hash", "kzg_eval", "kzg_quot", "kzg_msm"]
    assert signatures() == before
    dev.kzg_compute_proofs(blobs[:1], [K.fe(2)])
    assert [n for n, _ in dev.last_stage_times()] == ["kzg_eval", "kzg_quot", "kzg_msm"]
    dev.kzg_verify_blob_proof_batch(blobs, coms, proofs)
    assert [n for n, _ in dev.last_stage_times()] == ["kzg_hash", "kzg_eval", "kzg_tail"]


# ---- the MSM alone ---------------------------------------------------------------------
def lincomb_expected(a, job):
    return g1_of(sum(s * x for s, x in zip(job, a)) % R)


def sparse(pairs):
    v = [0] * N
    for i, s in pairs:
        v[i] = s
    return v


def test_lincomb_digit_and_group_law_edges(dev, setup_b):
    dev.kzg_load_setup_g1(setup_b)
    a = b_scalars()
    rng = random.Random(77)
    # digit exactly 128 in every window but the top (whose byte is lowered to stay below r), no
    # carry; and a carry chain through all 32 windows
    b80 = int.from_bytes(b"\x70" + b"\x80" * 31, "big")
    b81 = int.from_bytes(b"\x01" + b"\x81" * 31, "big")
    assert b80 < R and b81 < R
    jobs = [[0] * N, [1] * N, [R - 1] * N, [b80] * N, [b81] * N]
    for j in (0, 15, 31):
        for m in (128, 129):
            if m * 256 ** j < R:
                jobs.append([m * 256 ** j] * N)
    s = rng.randrange(R)
    jobs += [sparse([(0, s), (1, s)]),            # equal points, equal digits: the doubling branch
             sparse([(0, s), (2, s)]),            # opposite points: cancellation to infinity
             sparse([(0, 256), (3, 1)]),          # the same table point from two windows
             sparse([(0, 256 * s % R), (3, R - s)]),
             sparse([(5, s), (6, 1), (7, R - 1)]),  # the infinity points only
             sparse([(4, 1), (0, pow(2, 248, R))])]
    jobs += [[rng.randrange(R) for _ in range(N)] for _ in range(3)]
    out, st = dev.kzg_g1_lincomb([C.scalars_blob(j) for j in jobs])
    assert st == [OK] * len(jobs)
    exp = [lincomb_expected(a, j) for j in jobs]
    assert out == exp
    assert exp[0] == INF and exp[-8] == INF and exp[-6] == INF and exp[-5] == INF and exp[-9] != INF
    # a scalar = r names its job; the neighbour is still exact
    bad = list(jobs[-1])
    bad[N - 1] = R
    out, st = dev.kzg_g1_lincomb([C.scalars_blob(bad), C.scalars_blob(jobs[-1])])
    assert st == [BAD_SCALAR, OK] and out == [bytes(48), exp[-1]]


def test_lincomb_over_the_honest_setup(dev):
    rng = random.Random(78)
    job = [rng.randrange(R) for _ in range(N)]
    out, st = dev.kzg_g1_lincomb([C.scalars_blob(job)])
    assert st == [OK] and out == [S.commit(job)]


# ---- setup -----------------------------------------------------------------------------
def test_a_refused_g1_setup_keeps_the_old_one(dev, setup_a):
    cs = cases()[:2]
    blobs, want = [c[1] for c in cs], [c[2] for c in cs]
    x = 5
    while O.fp_sqrt((x ** 3 + 4) % O.P) is not None:
        x += 1
    off_curve = bytes([0x80 | (x >> 376)]) + x.to_bytes(48, "big")[1:]
    at = 1234
    good = setup_a[48 * at:48 * at + 48]
    outside = O.g1_to_bytes(O.g1_add(O.g1_from_bytes(good), H.torsion_point()))
    cleared = bytes([good[0] & 0x7F]) + good[1:]
    for bad, why in ((off_curve, "not on the curve"), (outside, "not in G1"), (cleared, "does not decode")):
        with pytest.raises(LodestarBlsError, match="G1 point %d .*%s" % (at, why)) as e:
            dev.kzg_load_setup_g1(setup_a[:48 * at] + bad + setup_a[48 * at + 48:])
        assert e.value.bad_index == at
        assert dev.kzg_setup_g1_loaded() is True
        assert dev.kzg_blob_commitments(blobs) == (want, [OK, OK])
    # the first bad point in file order is the one named
    two = setup_a[:48 * 7] + cleared + setup_a[48 * 8:48 * at] + off_curve + setup_a[48 * at + 48:]
    with pytest.raises(LodestarBlsError, match="G1 point 7 "):
        dev.kzg_load_setup_g1(two)


def test_mainnet_points_land_at_their_spec_indices(dev):
    with open(os.path.join(ROOT, "tests", "golden", "kzg_mainnet_g1_sample.json")) as f:
        sample = json.load(f)
    lines = [INF] * N
    for e in sample["points"]:
        lines[e["file_index"]] = bytes.fromhex(e["g1"])
    assert len(sample["points"]) == 64
    dev.kzg_load_setup_g1(b"".join(lines))
    rng = random.Random(79)
    f = [0] * N
    acc = None
    for e in sample["points"]:
        i = K.brp(e["file_index"])
        f[i] = rng.randrange(R)
        acc = O.g1_add(acc, O.g1_mul(O.g1_from_bytes(bytes.fromhex(e["g1"])), f[i]))
    coms, st = dev.kzg_blob_commitments([K.blob_from_ints(f)])
    assert st == [OK] and coms == [O.g1_to_bytes(acc)]


# ---- through the hosts -------------------------------------------------------------------
def write_setup_a(tmp_path, setup_a):
    path = tmp_path / "trusted_setup.txt"
    path.write_text(C.setup_text([setup_a[48 * i:48 * i + 48] for i in range(N)], S.tau_g2))
    return path


def test_gpu_kzg_commits_proves_and_verifies(dev, setup_a, tmp_path):
    g = kzg.GpuKzg(dev)
    g.load_trusted_setup(str(write_setup_a(tmp_path, setup_a)))
    f, blob, com, proof, _, _ = cases()[0]
    assert g.blob_to_kzg_commitment(blob) == com
    assert g.compute_blob_kzg_proof(blob, com) == proof
    assert g.verify_blob_kzg_proof(blob, g.blob_to_kzg_commitment(blob), g.compute_blob_kzg_proof(blob, com)) is True
    assert g.compute_kzg_proof(blob, K.fe(2)) == (S.proof(f, 2), K.fe(K.evaluate(f, 2)))
    assert g.blobs_to_kzg_commitments([c[1] for c in cases()[:3]]) == [c[2] for c in cases()[:3]]
    with pytest.raises(kzg.KzgError, match="item 0: BAD_BLOB"):
        g.blob_to_kzg_commitment(R.to_bytes(32, "big") + blob[32:])
    with pytest.raises(kzg.KzgError, match="item 0: BAD_COMMITMENT"):
        g.compute_blob_kzg_proof(blob, bytes(48))


def test_js_kzg_commit_through_the_addon(setup_a, tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "lodestar_amd", "napi", "lodestar_bls.node")
    if node is None or not os.path.exists(addon):
        pytest.skip("node or the addon not present")
    write_setup_a(tmp_path, setup_a)
    cs = cases()[:3]
    f, z = cs[0][0], 0x1CE1CE1CE % R
    files = {"blobs": [c[1] for c in cs], "commitments": [c[2] for c in cs], "proofs": [c[3] for c in cs],
             "z": [K.fe(z)], "y": [K.fe(K.evaluate(f, z))], "zproof": [S.proof(f, z)]}
    for name, items in files.items():
        (tmp_path / (name + ".bin")).write_bytes(b"".join(items))
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "kzg_commit_gpu.js"), str(tmp_path)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "kzg commit gpu ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
