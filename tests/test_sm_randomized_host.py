"""Randomized same-message aggregation, CPU side: the C ABI's new symbols, the Python
restatement of the mode (tests/sm_rand_helper.py) on the cancelling pair, and the option's
way from the verifiers to the device (the JS side: tests/test_js_sm_randomized.py).  No GPU.
"""
import asyncio
import ctypes
import hashlib
import os
import re

import pytest

import sm_rand_helper as H
from lodestar_amd import native
from oracle import batch as B
from oracle import bls12_381 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lb_set_same_message_mode", "lb_same_message_mode", "lb_same_message_aggregates")
SEEDS = [bytes(32), hashlib.sha256(b"sm-rand").digest()]


# ---- (a) symbols ---------------------------------------------------------------------
def test_header_and_library_have_the_new_entry_points():
    src = open(os.path.join(ROOT, "include", "lodestar_bls.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(native.library_path())
    for name in NEW_SYMBOLS:
        assert re.search(r"^\s*int\s+%s\s*\(" % name, src, flags=re.M), name
        assert name in native.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    for name, value in (("LB_SM_PLAIN", "0u"), ("LB_SM_RANDOMIZED", "1u"), ("LB_SM_AGG_INDEX_FLAG", "0x80000000u")):
        assert re.search(r"^#define\s+%s\s+%s\s*$" % (name, value), src, flags=re.M), name
    assert (native.LB_SM_PLAIN, native.LB_SM_RANDOMIZED, native.LB_SM_AGG_INDEX_FLAG) == (0, 1, 0x80000000)
    assert H.LB_SM_AGG_INDEX_FLAG == native.LB_SM_AGG_INDEX_FLAG


def test_null_context_is_refused_without_a_gpu():
    lib = native.load_library()
    assert lib.lb_set_same_message_mode(None, 1) == native.LB_ERR_INVALID_ARGUMENT
    assert lib.lb_same_message_mode(None) == native.LB_ERR_INVALID_ARGUMENT
    assert lib.lb_same_message_aggregates(None, None, None, None, None) == native.LB_ERR_INVALID_ARGUMENT


# ---- (b) the restatement -------------------------------------------------------------
@pytest.fixture(scope="module")
def signed():
    """Three keys, one root, their signatures, and the cancelling pair of the first two."""
    sks = [O.keygen(bytes([i + 1]) * 32) for i in range(3)]
    pks = [O.g1_to_bytes(O.sk_to_pk(sk), compressed=False) for sk in sks]
    root = hashlib.sha256(b"edge").digest()
    sigs = [O.g2_to_bytes(O.sign(sk, root)) for sk in sks]
    d = O.g2_mul(O.G2, 99991)
    s0 = O.g2_to_bytes(O.E2.add(O.signature_from_bytes(sigs[0]), d))
    s1 = O.g2_to_bytes(O.E2.add(O.signature_from_bytes(sigs[1]), O.E2.neg(d)))
    return pks, sigs, root, (s0, s1)


def test_agg_scalar_is_the_flagged_drbg_index():
    for seed in SEEDS:
        assert H.agg_scalar(seed, 5) == B.batch_scalar(seed, 0x80000005)
        assert H.agg_scalar(seed, 5) != B.batch_scalar(seed, 5)
    with pytest.raises(AssertionError):
        H.agg_scalar(SEEDS[0], 1 << 31)


def test_plain_sums_accept_the_cancelling_pair(signed):
    pks, _, root, pair = signed
    assert B.verify_same_message(list(zip(pks[:2], pair)), root) == ([True, True], True)


@pytest.mark.parametrize("seed", SEEDS, ids=["zero", "sha"])
def test_restatement_rejects_the_cancelling_pair(signed, seed):
    pks, sigs, root, pair = signed
    assert H.verify_same_message_randomized(list(zip(pks, sigs)), root, seed) == ([True, True, True], True)
    # as the job of a call's first two sets, and behind three other sets
    assert H.verify_same_message_randomized(list(zip(pks[:2], pair)), root, seed) == ([False, False], False)
    assert H.verify_same_message_randomized(list(zip(pks[:2], pair)), root, seed, index_base=3) == (
        [False, False], False)


def test_restatement_aggregates(signed):
    pks, sigs, root, _ = signed
    seed = SEEDS[1]
    inf = bytes([0xC0]) + bytes(95)
    jobs = [([], [], root), (pks[:1], sigs[:1], root), (pks[1:], sigs[1:], root),
            (pks[:2], [sigs[0], bytes([10]) * 96], root), (pks[:2], [inf, sigs[1]], root)]
    pk, sig, bad = H.randomized_aggregates(jobs, seed)
    assert bad == [True, False, False, True, False]
    assert pk[0] == bytes(96) and sig[0] == bytes(192) and pk[3] == bytes(96) and sig[3] == bytes(192)
    # a job of one set is not multiplied
    assert pk[1] == pks[0] and sig[1] == O.g2_to_bytes(O.signature_from_bytes(sigs[0]), compressed=False)
    # sets 1 and 2 of the call (the empty job holds none)
    r1, r2 = H.agg_scalar(seed, 1), H.agg_scalar(seed, 2)
    p = O.E1.add(O.g1_mul(O.g1_from_bytes(pks[1]), r1), O.g1_mul(O.g1_from_bytes(pks[2]), r2))
    assert pk[2] == O.g1_to_bytes(p, compressed=False)
    # the infinite signature contributes the identity: S = s_6 sig_1 (sets 5 and 6 of the call)
    s = O.g2_mul(O.signature_from_bytes(sigs[1]), H.agg_scalar(seed, 6))
    assert sig[4] == O.g2_to_bytes(s, compressed=False)


# ---- (c) the option reaches the device -------------------------------------------------
class FakeDev:
    """Stand-in for native.Device (no GPU): records the mode and what was submitted in it."""

    def __init__(self):
        self.mode_calls = []
        self.submitted = []
        self.closed = False

    def set_same_message_mode(self, randomized):
        self.mode_calls.append(bool(randomized))

    def verify_same_message_batch_async(self, jobs, seed, by_index=False):
        import numpy as np
        self.submitted.append((len(jobs), list(self.mode_calls)))
        return native.PendingSameMessage(0, len(jobs), None, None, np.zeros(1, np.uint32), list(jobs))

    def wait_same_message(self, pc):
        jobs = pc.keep
        return ([[True] * len(s) for _, s, _ in jobs], [True] * len(jobs), (0, sum(len(s) for _, s, _ in jobs)),
                0.0)

    def last_stage_times(self):
        return []

    def close(self):
        self.closed = True


def test_option_reaches_the_device_through_the_verifiers():
    from lodestar_amd.verifier import BlsGpuSingleThreadVerifier, BlsGpuVerifier, DeviceBackend, PublicKey

    async def main(randomized):
        dev = FakeDev()
        b = DeviceBackend(seed_source=lambda: bytes(32), dev=dev, capacity=2, same_message_randomized=randomized)
        assert b.same_message_randomized is randomized
        v = BlsGpuVerifier(backends=[b])
        sets = [(PublicKey(bytes([7]) * 96), bytes(96)) for _ in range(3)]
        assert await v.verify_signature_sets_same_message(sets, bytes(32)) == [True, True, True]
        await v.close()
        return dev
    dev = asyncio.run(main(True))
    # the mode was set once, before the first package went out
    assert dev.mode_calls == [True] and dev.submitted == [(1, [True])] and dev.closed
    dev = asyncio.run(main(False))
    assert dev.mode_calls == [] and dev.submitted == [(1, [])]  # the default leaves the context's mode
    # the single-thread verifier inherits it through its backend
    dev = FakeDev()
    st = BlsGpuSingleThreadVerifier(DeviceBackend(seed_source=lambda: bytes(32), dev=dev, capacity=1,
                                                  same_message_randomized=True))
    assert st.backend.same_message_randomized and dev.mode_calls == [True]
    asyncio.run(st.close())
