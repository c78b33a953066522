"""Per-job aggregate signatures on the GPU (lb_verify_same_message_batch_agg, k_aggsig.hip) and
grouped signature aggregation (lb_aggregate_signature_groups).

Each job's output is compared byte for byte with the Python restatement
(tests/sm_agg_helper.py: Signature.aggregate(valid, unmasked sets).toBytes()); verdicts are
known by construction (a signature over the job's root by the set's key is valid, one over
another root is not), and verdicts / fast flags / stats are compared with
lb_verify_same_message_batch on the same input.
"""
import asyncio
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sm_agg_helper as A  # noqa: E402
import workloads as W  # noqa: E402
from lodestar_amd import native  # noqa: E402
from lodestar_amd.verifier import BlsGpuSingleThreadVerifier, BlsGpuVerifier, DeviceBackend, PublicKey  # noqa: E402
from oracle import bls12_381 as O  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = [bytes(32), hashlib.sha256(b"sm-agg").digest()]
MALFORMED = bytes([10]) * 96
# TPB = 64: both sides of one wave and of two, and a job of several tiles; one empty job
SIZES = [1, 2, 3, 63, 64, 65, 128, 129, 200, 0]


def root_of(tag: bytes) -> bytes:
    return hashlib.sha256(b"sm-agg" + tag).digest()


@pytest.fixture(scope="module")
def keyed():
    dev = native.Device(0)
    keys = W.make_keys(dev, 1024)
    assert dev.pubkey_table_append(keys.pks) == len(keys.pks)
    yield dev, keys
    dev.close()


@pytest.fixture(params=[False, True], ids=["plain", "randomized"])
def mode(request, keyed):
    dev, _ = keyed
    dev.set_same_message_mode(request.param)
    yield request.param
    dev.set_same_message_mode(False)


def honest_job(dev, keys, ix, root):
    """(validator indices, their signatures over root, root)"""
    return list(ix), W.sign_many(dev, [keys.sks[i] for i in ix], [root] * len(ix)), root


def by_bytes(keys, jobs):
    return [([keys.pks[i] for i in ix], sigs, m) for ix, sigs, m in jobs]


def not_in_subgroup_signature() -> bytes:
    """An on-curve G2 point outside the subgroup, compressed: y = sqrt(x^3 + 4(1 + u)) for the first
    small x that has one, no cofactor clearing."""
    for k in range(1, 64):
        x = (k, 1)
        y = O.f2_sqrt(O.f2_add(O.f2_mul(O.f2_sqr(x), x), (4, 4)))
        if y is not None and not O.g2_in_subgroup((x, y)):
            return O.g2_to_bytes((x, y))
    raise AssertionError("no point found")


def cancelling_pair(sig0: bytes, sig1: bytes, k: int = 99991):
    """sig0 + D and sig1 - D, D = [k] G2 (tests/test_gpu_sm_randomized.py::cancelling_pair)."""
    d = O.g2_mul(O.G2, k)
    return (O.g2_to_bytes(O.E2.add(O.signature_from_bytes(sig0), d)),
            O.g2_to_bytes(O.E2.add(O.signature_from_bytes(sig1), O.E2.neg(d))))


def check_against_plain_call(dev, jobs, seed, got, **kw):
    """verdicts, fast flags and stats of the _agg call = those of lb_verify_same_message_batch"""
    res, fast, stats = dev.verify_same_message_batch(jobs, seed, **kw)
    assert got[0] == res and got[1] == fast and dev.last_stats == stats
    return res


# ---- bit-exact sums ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sized_package(keyed):
    dev, keys = keyed
    jobs, v = [], 0
    for j, n in enumerate(SIZES):
        jobs.append(honest_job(dev, keys, range(v, v + n), root_of(bytes([j]))))
        v += n
    jobs = by_bytes(keys, jobs)
    want = A.expected_job_aggregates(jobs, [[True] * n for n in SIZES], validate=False)
    return jobs, want


@pytest.mark.parametrize("seed", SEEDS, ids=["zero", "sha"])
def test_sums_bit_exact(keyed, mode, sized_package, seed):
    dev, _ = keyed
    jobs, want = sized_package
    # a condition on the inputs: both values of the compression sign bit are exercised
    assert {w[0][0] & 0x20 for w, n in zip(want, SIZES) if n} == {0, 0x20}
    res, fast, sigs, counts = dev.verify_same_message_batch(jobs, seed, aggregate=True)
    assert res == [[True] * n for n in SIZES] and fast == [n > 0 for n in SIZES]
    for j in range(len(SIZES)):
        assert (sigs[j], counts[j]) == want[j], j
    assert sigs[-1] == A.INFINITY96 and counts[-1] == 0
    assert "sm_job_sig" in [n for n, _ in dev.last_stage_times(raw=True, limit=40)]


# ---- retry path ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def retry_package(keyed):
    """(jobs by bytes, verdicts in the plain mode, verdicts in the randomized mode)"""
    dev, keys = keyed
    jobs, plain = [], []
    r = [root_of(b"retry" + bytes([j])) for j in range(6)]
    other = root_of(b"another root")
    ix, s, _ = honest_job(dev, keys, range(700, 705), r[0])
    s[2] = W.sign_many(dev, [keys.sks[702]], [other])[0]  # a wrong-root signature in the middle
    jobs.append((ix, s, r[0]))
    plain.append([True, True, False, True, True])
    ix, s, _ = honest_job(dev, keys, range(705, 708), r[1])
    s[1] = MALFORMED
    jobs.append((ix, s, r[1]))
    plain.append([True, False, True])
    ix, s, _ = honest_job(dev, keys, range(708, 711), r[2])
    s[0] = not_in_subgroup_signature()
    jobs.append((ix, s, r[2]))
    plain.append([False, True, True])
    ix = [711, 712]
    jobs.append((ix, W.sign_many(dev, [keys.sks[i] for i in ix], [other] * 2), r[3]))  # every set invalid
    plain.append([False, False])
    ix, s, _ = honest_job(dev, keys, range(713, 716), r[4])
    s[0], s[2] = cancelling_pair(s[0], s[2])
    jobs.append((ix, s, r[4]))
    plain.append([True, True, True])  # the plain sums accept the pair
    jobs.append(honest_job(dev, keys, range(716, 786), r[5]))  # a clean job of 70 sets beside them
    plain.append([True] * 70)
    rand = [list(v) for v in plain]
    rand[4] = [False, True, False]
    return by_bytes(keys, jobs), plain, rand


def test_retry_path(keyed, mode, retry_package):
    dev, _ = keyed
    jobs, plain, rand = retry_package
    verdicts = rand if mode else plain
    got = dev.verify_same_message_batch(jobs, SEEDS[1], aggregate=True)
    assert got[0] == verdicts
    assert got[1] == [False, False, False, False, not mode, True]
    check_against_plain_call(dev, jobs, SEEDS[1], got)
    want = A.expected_job_aggregates(jobs, verdicts, validate=False)
    for j in range(len(jobs)):
        assert (got[2][j], got[3][j]) == want[j], j
    assert (got[2][3], got[3][3]) == (A.INFINITY96, 0)  # every set invalid
    if mode:
        assert got[3][4] == 1  # both sets of the cancelling pair are left out


# ---- mask ----------------------------------------------------------------------------------
def test_mask(keyed, mode):
    dev, keys = keyed
    r = [root_of(b"mask" + bytes([j])) for j in range(3)]
    j0 = honest_job(dev, keys, range(800, 806), r[0])
    j1 = honest_job(dev, keys, range(806, 871), r[1])
    ix, s, _ = honest_job(dev, keys, range(871, 876), r[2])
    s[3] = W.sign_many(dev, [keys.sks[874]], [r[0]])[0]  # a retry in the masked job
    jobs = by_bytes(keys, [j0, j1, (ix, s, r[2])])
    verdicts = [[True] * 6, [True] * 65, [True, True, True, False, True]]
    mask = [[False] * 6, [i % 3 != 1 for i in range(65)], [True, False, True, True, False]]
    got = dev.verify_same_message_batch(jobs, SEEDS[0], aggregate=True, mask=mask)
    assert got[0] == verdicts and got[1] == [True, True, False]  # masked-out sets keep their verdicts
    check_against_plain_call(dev, jobs, SEEDS[0], got)
    want = A.expected_job_aggregates(jobs, verdicts, mask, validate=False)
    assert [(s, c) for s, c in zip(got[2], got[3])] == want
    assert want[0] == (A.INFINITY96, 0) and want[1][1] == 43 and want[2][1] == 2


# ---- pubkey-table forms --------------------------------------------------------------------
def test_by_index_and_mixed_packages(keyed, mode):
    dev, keys = keyed
    r = [root_of(b"table" + bytes([j])) for j in range(3)]
    j0 = honest_job(dev, keys, range(900, 904), r[0])
    ix, s, _ = honest_job(dev, keys, range(904, 907), r[1])
    s[1] = W.sign_many(dev, [keys.sks[905]], [r[0]])[0]
    j1 = (ix, s, r[1])
    verdicts = [[True] * 4, [True, False, True]]
    got = dev.verify_same_message_batch([j0, j1], SEEDS[1], by_index=True, aggregate=True)
    assert got[0] == verdicts
    check_against_plain_call(dev, [j0, j1], SEEDS[1], got, by_index=True)
    want = A.expected_job_aggregates([j0, j1], verdicts, validate=False)
    assert list(zip(got[2], got[3])) == want
    # mixed: keys 907 and 908 travel as rows (96-byte and 48-byte compressed), 909 by index
    rows = keys.pks[907] + O.g1_to_bytes(O.g1_from_bytes(keys.pks[908]), compressed=True) + bytes(48)
    _, s, _ = honest_job(dev, keys, [907, 908, 909], r[2])
    j2 = ([native.LB_PK_ROW_FLAG | 0, native.LB_PK_ROW_FLAG | native.LB_PK_ROW48_FLAG | 1, 909], s, r[2])
    b, out, fast, job_off, keep = dev._same_message_batch([j0, j2], SEEDS[1], True, rows)
    sig96, count, _ = dev._agg_arrays(2, 7, None)
    st = native._Stats()
    rc = dev.lib.lb_verify_same_message_batch_agg(dev._h, ctypes.byref(b), None, out.ctypes.data, fast.ctypes.data,
                                                  sig96.ctypes.data, count.ctypes.data, ctypes.byref(st))
    assert rc == native.LB_OK and out[:7].tolist() == [1] * 7 and fast[:2].tolist() == [1, 1]
    want = A.expected_job_aggregates([j0, j2], [[True] * 4, [True] * 3], validate=False)
    raw = sig96.tobytes()
    assert [(raw[:96], int(count[0])), (raw[96:192], int(count[1]))] == want


# ---- async ---------------------------------------------------------------------------------
def test_async_more_packages_than_slots(keyed, mode):
    dev, keys = keyed
    n = dev.slots() + 2
    other = root_of(b"async other")
    packages, verdicts, masks = [], [], []
    for p in range(n):
        root = root_of(b"async" + bytes([p]))
        ix, s, _ = honest_job(dev, keys, range(40 * p, 40 * p + 3 + p), root)
        v = [True] * len(ix)
        if p % 2:  # every other package carries a retry
            s[1] = W.sign_many(dev, [keys.sks[ix[1]]], [other])[0]
            v[1] = False
        small = honest_job(dev, keys, [40 * p + 30, 40 * p + 31], root_of(b"async small" + bytes([p])))
        packages.append(by_bytes(keys, [(ix, s, root), small]))
        verdicts.append([v, [True, True]])
        masks.append(None if p % 3 else [[i != 0 for i in range(len(ix))], [True, False]])
    pending = [dev.verify_same_message_batch_async(pk, SEEDS[1], aggregate=True, mask=m)
               for pk, m in zip(packages, masks)]
    for p in reversed(range(n)):  # waited for out of submission order
        res, fast, sigs, counts = dev.wait_same_message(pending[p])
        assert res == verdicts[p] and fast == [all(v) for v in verdicts[p]], p
        want = A.expected_job_aggregates(packages[p], verdicts[p], masks[p], validate=False)
        assert list(zip(sigs, counts)) == want, p


# ---- closure: the returned signature verifies as the aggregate it claims to be ---------------
def test_returned_aggregates_verify(keyed, mode):
    dev, keys = keyed
    roots = [root_of(b"closure" + bytes([j])) for j in range(3)]
    other = root_of(b"closure other")
    jobs = [honest_job(dev, keys, range(950, 953), roots[0]), honest_job(dev, keys, range(953, 1020), roots[1])]
    ix, s, _ = honest_job(dev, keys, range(1020, 1024), roots[2])
    s[2] = W.sign_many(dev, [keys.sks[1022]], [other])[0]
    jobs.append((ix, s, roots[2]))
    mask = [[True, False, True], [True] * 67, [True] * 4]
    res, _, sigs, counts = dev.verify_same_message_batch(by_bytes(keys, jobs), SEEDS[1], aggregate=True, mask=mask)
    included = [[i for k, i in enumerate(ix) if res[j][k] and mask[j][k]] for j, (ix, _, _) in enumerate(jobs)]
    assert counts == [2, 67, 3] == [len(i) for i in included]
    pks = b"".join(dev.aggregate_pubkeys([keys.pks[i] for i in inc]) for inc in included)
    blob, offs = native.pack_blobs(sigs)
    out = dev.verify_requests(np.arange(4, dtype=np.uint32), np.frombuffer(pks, np.uint8), None,
                              np.frombuffer(b"".join(roots), np.uint8), blob, offs, SEEDS[0])
    assert out.valid.tolist() == [1, 1, 1] and out.errors.tolist() == [0, 0, 0]


# ---- groups --------------------------------------------------------------------------------
def test_signature_groups(keyed):
    dev, keys = keyed
    root = root_of(b"groups")
    sizes = [1, 2, 64, 65, 129]
    sigs = W.sign_many(dev, keys.sks[:sum(sizes)], [root] * sum(sizes))
    groups, v = [], 0
    for n in sizes:
        groups.append(sigs[v:v + n])
        v += n
    want = ([A.aggregate_bytes(g, validate=False) for g in groups], [-1] * len(sizes))
    assert dev.aggregate_signature_groups(groups) == want
    assert dev.aggregate_signature_groups(groups, no_check=True) == want
    # a signature outside the subgroup: reported by default, summed with LB_AGG_NO_CHECK
    rogue = not_in_subgroup_signature()
    bad = [sigs[:3], [sigs[3], rogue, sigs[4]], [sigs[5], MALFORMED], sigs[6:71]]
    assert dev.aggregate_signature_groups(bad) == A.expected_groups(bad)
    assert dev.aggregate_signature_groups(bad)[1] == [-1, 4, 7, -1]
    got = dev.aggregate_signature_groups(bad, no_check=True)
    assert got == A.expected_groups(bad, no_check=True)
    assert got[1] == [-1, -1, 7, -1] and got[0][1] != bytes(96) and got[0][2] == bytes(96)
    with pytest.raises(native.EmptyAggregateError):
        dev.aggregate_signature_groups([sigs[:2], []])
    goff = np.array([0, 2, 2], np.uint32)
    blob, offs = native.pack_blobs(sigs[:2])
    out, bi = np.zeros(192, np.uint8), np.zeros(2, np.int32)
    assert dev.lib.lb_aggregate_signature_groups(dev._h, 2, goff.ctypes.data, blob.ctypes.data, offs.ctypes.data, 0,
                                                 out.ctypes.data, bi.ctypes.data) == native.LB_ERR_INVALID_ARGUMENT


# ---- hosts ---------------------------------------------------------------------------------
def four_set_job():
    """A 4-set job whose third set is signed over another root: (96-byte keys, signatures, root)."""
    sks = [O.keygen(bytes([i + 60]) * 32) for i in range(4)]
    pks = [O.g1_to_bytes(O.sk_to_pk(sk), compressed=False) for sk in sks]
    root = bytes([78]) * 32
    sigs = [O.g2_to_bytes(O.sign(sk, root)) for sk in sks]
    sigs[2] = O.g2_to_bytes(O.sign(sks[2], bytes([79]) * 32))
    return pks, sigs, root


def test_hosts_python():
    pks, sigs, root = four_set_job()
    sets = [(PublicKey(p), s) for p, s in zip(pks, sigs)]
    include = [True, False, True, True]

    async def main():
        b = DeviceBackend(0, seed_source=lambda: SEEDS[1])
        v = BlsGpuVerifier(backends=[b])
        everything = await v.verify_and_aggregate_same_message(sets, root)
        masked = await v.verify_and_aggregate_same_message(sets, root, include=include)
        plain = await v.verify_signature_sets_same_message(sets, root)
        st = BlsGpuSingleThreadVerifier(b)
        single = await st.verify_and_aggregate_same_message(sets, root, include=include)
        await v.close()
        return everything, masked, plain, single
    everything, masked, plain, single = asyncio.run(main())
    valid = [True, True, False, True]
    assert plain == valid
    assert everything == (valid, A.aggregate_bytes([sigs[0], sigs[1], sigs[3]]), 3)
    assert masked == single == (valid, A.aggregate_bytes([sigs[0], sigs[3]]), 2)


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
    pks, sigs, root = four_set_job()
    inp = tmp_path / "job.json"
    inp.write_text(json.dumps({"pks": [p.hex() for p in pks], "sigs": [s.hex() for s in sigs], "root": root.hex(),
                               "include": [True, False, True, True], "groups": [[0, 1], [3]]}))
    r = subprocess.run([node, os.path.join(ROOT, "tests", "js", "sm_aggregate_gpu.js"), str(inp)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    valid = [True, True, False, True]
    assert out["plain"] == valid
    assert out["all"] == {"valid": valid, "signature": A.aggregate_bytes([sigs[0], sigs[1], sigs[3]]).hex(), "count": 3}
    masked = {"valid": valid, "signature": A.aggregate_bytes([sigs[0], sigs[3]]).hex(), "count": 2}
    assert out["masked"] == masked and out["single"] == masked
    assert out["groups"] == [A.aggregate_bytes(sigs[:2]).hex(), sigs[3].hex()]


# ---- plain calls are as they were ----------------------------------------------------------
def test_plain_call_runs_no_sm_job_sig(keyed):
    dev, keys = keyed
    job = by_bytes(keys, [honest_job(dev, keys, range(4), root_of(b"plain"))])
    res, fast, _ = dev.verify_same_message_batch(job, SEEDS[0])
    assert res == [[True] * 4] and fast == [True]
    names = [n for n, _ in dev.last_stage_times(raw=True, limit=40)]
    assert names and "sm_job_sig" not in names
