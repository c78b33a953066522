"""Randomized same-message aggregation on the GPU (LB_SM_RANDOMIZED, k_smrand.hip).

Every job of >= 2 sets is aggregated as sum s_i pk_i / sum s_i sig_i with
s_i = batch_scalar(seed, 0x80000000 | i), so a passing aggregate implies every set valid:
the cancelling pair sig_0 + D, sig_1 - D that the plain sums accept is rejected.  The
aggregates are compared byte for byte with the Python restatement (tests/sm_rand_helper.py),
the verdicts with each set verified alone.
"""
import asyncio
import hashlib
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import sm_rand_helper as H  # noqa: E402
import workloads as W  # noqa: E402
from lodestar_amd import native  # noqa: E402
from lodestar_amd.verifier import BlsGpuVerifier, DeviceBackend, PublicKey  # noqa: E402
from oracle import bls12_381 as O  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = [bytes(32), hashlib.sha256(b"sm-rand").digest()]
INF_SIG = bytes([0xC0]) + bytes(95)
MALFORMED = bytes([10]) * 96


@pytest.fixture(scope="module")
def keyed():
    dev = native.Device(0)
    keys = W.make_keys(dev, 16384)
    assert dev.pubkey_table_append(keys.pks) == len(keys.pks)
    yield dev, keys
    dev.close()


def cancelling_pair(sig0: bytes, sig1: bytes, k: int = 99991):
    """sig0 + D and sig1 - D, D = [k] G2: both individually invalid, their sum unchanged."""
    d = O.g2_mul(O.G2, k)
    return (O.g2_to_bytes(O.E2.add(O.signature_from_bytes(sig0), d)),
            O.g2_to_bytes(O.E2.add(O.signature_from_bytes(sig1), O.E2.neg(d))))


def pair_job(dev, keys, a: int, b: int, root: bytes):
    """A by-index job of validators a, b over `root` holding the cancelling pair."""
    s = W.sign_many(dev, [keys.sks[a], keys.sks[b]], [root, root])
    return [a, b], list(cancelling_pair(s[0], s[1])), root


@pytest.fixture(scope="module")
def agg_package(keyed):
    """Jobs of 0, 1, 2, 64, 65 and 129 sets by table index (TPB = 64: the empty job, the
    unmultiplied single, the smallest sum, a full wave, one set past it -- the tree's
    partial-range guard -- and two strides plus one), and small jobs with a malformed
    signature, the infinite signature, a key as a 96-byte row and as a 48-byte compressed row.
    Returns (jobs by index, rows, the same jobs with every key as bytes)."""
    dev, keys = keyed
    sizes = [0, 1, 2, 64, 65, 129]
    roots = [hashlib.sha256(b"sm-rand-agg" + bytes([j])).digest() for j in range(len(sizes) + 4)]
    jobs, v = [], 0
    for j, n in enumerate(sizes):
        ix = list(range(v, v + n))
        v += n
        jobs.append((ix, W.sign_many(dev, [keys.sks[i] for i in ix], [roots[j]] * n), roots[j]))
    ix = [v, v + 1, v + 2]
    s = W.sign_many(dev, [keys.sks[i] for i in ix], [roots[6]] * 3)
    jobs.append((ix, [s[0], MALFORMED, s[2]], roots[6]))
    jobs.append((ix, [s[0], INF_SIG, s[2]], roots[7]))
    # mixed package: rows of the call's own key bytes, named by flagged indices
    rows = keys.pks[v + 3] + O.g1_to_bytes(O.g1_from_bytes(keys.pks[v + 4]), compressed=True) + bytes(48)
    s8 = W.sign_many(dev, [keys.sks[v + 3], keys.sks[v + 5]], [roots[8]] * 2)
    jobs.append(([native.LB_PK_ROW_FLAG | 0, v + 5], s8, roots[8]))
    s9 = W.sign_many(dev, [keys.sks[v + 6], keys.sks[v + 4]], [roots[9]] * 2)
    jobs.append(([v + 6, native.LB_PK_ROW_FLAG | native.LB_PK_ROW48_FLAG | 1], s9, roots[9]))

    def key_bytes(i):
        if i & native.LB_PK_ROW_FLAG:
            r = i & native.LB_PK_ROW_MASK
            return rows[96 * r:96 * r + (48 if i & native.LB_PK_ROW48_FLAG else 96)]
        return keys.pks[i]
    by_bytes = [([key_bytes(i) for i in ix], sg, m) for ix, sg, m in jobs]
    return jobs, rows, by_bytes


@pytest.mark.parametrize("seed", SEEDS, ids=["zero", "sha"])
def test_aggregates_bit_exact(keyed, agg_package, seed):
    dev, _ = keyed
    jobs, rows, by_bytes = agg_package
    dev.set_same_message_mode(True)
    try:
        assert dev.same_message_mode == native.LB_SM_RANDOMIZED
        got = dev.same_message_aggregates(jobs, seed, by_index=True, rows=rows)
    finally:
        dev.set_same_message_mode(False)
    want = H.randomized_aggregates(by_bytes, seed)
    assert got[2] == want[2] == [True, False, False, False, False, False, True, False, False, False]
    for j in range(len(jobs)):
        assert got[0][j] == want[0][j], ("pk", j)
        assert got[1][j] == want[1][j], ("sig", j)
    # back in the plain mode: the plain sums
    assert dev.same_message_mode == native.LB_SM_PLAIN
    pk, sig, bad = dev.same_message_aggregates(jobs, seed, by_index=True, rows=rows)
    assert bad == want[2]
    for j, (pks, sigs, _) in enumerate(by_bytes):
        if bad[j]:
            assert pk[j] == bytes(96) and sig[j] == bytes(192)
            continue
        assert pk[j] == O.g1_to_bytes(O.aggregate_g1([O.g1_from_bytes(p) for p in pks]), compressed=False), j
        assert sig[j] == O.g2_to_bytes(O.aggregate_g2([O.signature_from_bytes(s) for s in sigs]),
                                       compressed=False), j


@pytest.mark.parametrize("seed", SEEDS, ids=["zero", "sha"])
def test_cancelling_pair_rejected(keyed, seed):
    dev, keys = keyed
    root = hashlib.sha256(b"edge").digest()
    honest = ([2, 3, 4], W.sign_many(dev, keys.sks[2:5], [root] * 3), root)
    jobs = [pair_job(dev, keys, 0, 1, root), honest]
    dev.set_same_message_mode(True)
    try:
        res, fast, (retried, ok_sets) = dev.verify_same_message_batch(jobs, seed, by_index=True)
    finally:
        dev.set_same_message_mode(False)
    assert res == [[False, False], [True, True, True]]
    assert fast == [False, True]
    assert (retried, ok_sets) == (1, 3)
    # the same Device, plain again: the plain sums accept the pair
    res, fast, _ = dev.verify_same_message_batch(jobs[:1], seed, by_index=True)
    assert res == [[True, True]] and fast == [True]


def test_verdict_parity_with_sets_alone(keyed):
    """Every set's verdict equals the set verified alone (C oracle), by index and by bytes."""
    from oracle import c_oracle as C
    dev, keys = keyed
    jobs, expect = W.same_message_jobs(dev, keys, n_jobs=24, per_job=32, seed=5, n_invalid=9)
    for k in range(3):
        root = hashlib.sha256(b"sm-rand-pair" + bytes([k])).digest()
        jobs.append(pair_job(dev, keys, 100 + 2 * k, 101 + 2 * k, root))
        expect.append([False, False])
    flat = [(keys.pks[i], s, m) for ix, sigs, m in jobs for i, s in zip(ix, sigs)]
    blob, offs = native.pack_blobs([s for _, s, _ in flat])
    n = len(flat)
    valid, _ = C.verify_requests(np.arange(n + 1, dtype=np.uint32),
                                 np.frombuffer(b"".join(p for p, _, _ in flat), np.uint8), None,
                                 np.frombuffer(b"".join(m for _, _, m in flat), np.uint8), blob, offs, bytes(32),
                                 threads=16)
    alone = [bool(x) for x in valid]
    assert alone == [v for e in expect for v in e]
    by_bytes = [([keys.pks[i] for i in ix], s, m) for ix, s, m in jobs]
    dev.set_same_message_mode(True)
    try:
        out_i = dev.verify_same_message_batch(jobs, bytes(32), by_index=True)
        out_b = dev.verify_same_message_batch(by_bytes, bytes(32))
    finally:
        dev.set_same_message_mode(False)
    for res, fast, (retried, ok_sets) in (out_i, out_b):
        assert [v for r in res for v in r] == alone
        assert fast == [all(r) for r in res]
        assert retried == sum(1 for f in fast if not f)
        assert ok_sets == sum(len(r) for r, f in zip(res, fast) if f)


def test_mode_is_captured_at_submit(keyed):
    dev, keys = keyed
    root = hashlib.sha256(b"sm-rand-async").digest()
    pair = pair_job(dev, keys, 0, 1, root)
    honest = ([2, 3], W.sign_many(dev, keys.sks[2:4], [root] * 2), root)
    dev.set_same_message_mode(True)
    try:
        p1 = dev.verify_same_message_batch_async([pair, honest], SEEDS[1], by_index=True)
    finally:
        dev.set_same_message_mode(False)
    p2 = dev.verify_same_message_batch_async([pair, honest], SEEDS[1], by_index=True)
    res1, fast1, _, _ = dev.wait_same_message(p1)
    res2, fast2, _, _ = dev.wait_same_message(p2)
    assert res1 == [[False, False], [True, True]] and fast1 == [False, True]
    assert res2 == [[True, True], [True, True]] and fast2 == [True, True]


def test_natural_size_package(keyed):
    """512 jobs x 128 sets with 40 corrupted sets, and cancelling pairs in 8 jobs."""
    dev, keys = keyed
    jobs, expect = W.same_message_jobs(dev, keys, n_jobs=512, per_job=128, n_invalid=40)
    clean = [j for j, e in enumerate(expect) if all(e)][:8]
    for j in clean:
        ix, sigs, _ = jobs[j]
        sigs[5], sigs[70] = cancelling_pair(sigs[5], sigs[70], 7919 + j)
        expect[j][5] = expect[j][70] = False
    dev.set_same_message_mode(True)
    try:
        res, fast, (retried, ok_sets) = dev.verify_same_message_batch(jobs, SEEDS[1], by_index=True)
    finally:
        dev.set_same_message_mode(False)
    assert res == expect
    bad_jobs = {j for j, e in enumerate(expect) if not all(e)}
    assert set(clean) <= bad_jobs
    assert [not f for f in fast] == [j in bad_jobs for j in range(512)]
    assert retried == len(bad_jobs) and ok_sets == 128 * (512 - len(bad_jobs))


def four_set_job():
    """A 4-set job whose first two sets are a cancelling pair: (96-byte keys, signatures, root)."""
    sks = [O.keygen(bytes([i + 40]) * 32) for i in range(4)]
    pks = [O.g1_to_bytes(O.sk_to_pk(sk), compressed=False) for sk in sks]
    root = bytes([77]) * 32
    sigs = [O.g2_to_bytes(O.sign(sk, root)) for sk in sks]
    sigs[0], sigs[1] = cancelling_pair(sigs[0], sigs[1])
    return pks, sigs, root


def test_hosts_python():
    pks, sigs, root = four_set_job()

    async def main():
        b = DeviceBackend(0, seed_source=lambda: SEEDS[1], same_message_randomized=True)
        assert b.dev.same_message_mode == native.LB_SM_RANDOMIZED
        v = BlsGpuVerifier(backends=[b])
        out = await v.verify_signature_sets_same_message([(PublicKey(p), s) for p, s in zip(pks, sigs)], root)
        # lb_verify_same_message (one job) on the same context
        one, used_fast = b.dev.verify_same_message(pks, sigs, root, SEEDS[1])
        await v.close()
        return out, [bool(x) for x in one], used_fast
    out, one, used_fast = asyncio.run(main())
    assert out == [False, False, True, True]
    assert one == [False, False, True, True] and not used_fast


def test_hosts_js_addon(tmp_path):
    node = shutil.which("node")
    addon = os.path.join(ROOT, "lodestar_amd", "napi", "lodestar_bls.node")
    if node is None:
        pytest.skip("node not installed")
    if not os.path.exists(addon):
        from lodestar_amd.napi import build as nb
        if not nb.available():
            pytest.skip("node headers not available")
        nb.build()
    import json
    pks, sigs, root = four_set_job()
    inp = tmp_path / "job.json"
    inp.write_text(json.dumps({"pks": [p.hex() for p in pks], "sigs": [s.hex() for s in sigs], "root": root.hex()}))
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "sm_randomized_gpu.js"), str(inp)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["randomized"] == [False, False, True, True]
    assert out["plain"] == [True, True, True, True]


def test_randomized_refuses_calls_reaching_the_index_flag(keyed):
    """n_sets >= 2^31 would reach LB_SM_AGG_INDEX_FLAG: refused before anything is read."""
    import ctypes
    dev, _ = keyed
    job_off = np.array([0, 1 << 31], np.uint32)
    one = np.zeros(32, np.uint8)
    offs = np.zeros(2, np.uint32)
    b = native._SameMessageBatch(1, 1 << 31, job_off.ctypes.data, one.ctypes.data, None, one.ctypes.data,
                                 offs.ctypes.data, one.ctypes.data, one.ctypes.data)
    out = np.zeros(192, np.uint8)
    dev.set_same_message_mode(True)
    try:
        rc = dev.lib.lb_same_message_aggregates(dev._h, ctypes.byref(b), out.ctypes.data, out.ctypes.data,
                                                out.ctypes.data)
        assert rc == native.LB_ERR_INVALID_ARGUMENT
        rc = dev.lib.lb_verify_same_message_batch(dev._h, ctypes.byref(b), out.ctypes.data, None, None)
        assert rc == native.LB_ERR_INVALID_ARGUMENT
        assert b"2^31" in dev.lib.lb_last_error(dev._h)
    finally:
        dev.set_same_message_mode(False)


def test_bad_mode_is_refused(keyed):
    dev, _ = keyed
    assert dev.lib.lb_set_same_message_mode(dev._h, 2) == native.LB_ERR_INVALID_ARGUMENT
    assert dev.same_message_mode == native.LB_SM_PLAIN
    dev.set_same_message_mode(True)
    try:
        assert dev.lib.lb_set_same_message_mode(dev._h, 2) == native.LB_ERR_INVALID_ARGUMENT
        assert dev.same_message_mode == native.LB_SM_RANDOMIZED
    finally:
        dev.set_same_message_mode(False)
