"""The synchronous helper calls that take their buffers from slot 0's slab per call (the KZG
calls, the shuffle, the sampling; lodestar_amd/csrc/bls_host.hip HelperCall): calls of different
kinds and sizes sharing the slab on one context, the per-item pass of a failed KZG batch behind
a call of another size, the MSM's group buffers at one job and past a group, and a context whose
stage events are switched off.  Every comparison is exact."""
import hashlib
import os
import re

import numpy as np
import pytest

import sample_helper as SA
import shuffle_helper as SH
from lodestar_amd.native import Device, pack_blobs
from tests import kzg_commit_helper as C
from tests import kzg_helper as K

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "lodestar_amd", "csrc", "bls_kzg.h")) as _f:
    MSM_GROUP = int(re.search(r"LB_KZG_MSM_GROUP = (\d+);", _f.read()).group(1))
N = K.N
S = K.TestSetup()
OK = 0


@pytest.fixture(scope="module")
def sidecars():
    """Three honest (blob, commitment, proof)."""
    return [S.blob_case(K.random_poly(100 + i))[:3] for i in range(3)]


@pytest.fixture(scope="module")
def g1_setup():
    """The honest setup's G1 lines in file order, its points made on the GPU."""
    d = Device(0)
    try:
        lag = C.lagrange_scalars(S.tau)
        pks = d.sk_to_pk([(s if s else 1).to_bytes(32, "big") for s in lag])
    finally:
        d.close()
    return b"".join(C.file_order([C.g1_compress(p) if s else K.G1_INF for p, s in zip(pks, lag)]))


def kzg_device(g1_setup, stage_events=True):
    old = os.environ.get("LB_STAGE_EVENTS")
    os.environ["LB_STAGE_EVENTS"] = "1" if stage_events else "0"
    try:
        d = Device(0)
    finally:
        if old is None:
            del os.environ["LB_STAGE_EVENTS"]
        else:
            os.environ["LB_STAGE_EVENTS"] = old
    d.kzg_load_setup(S.tau_g2)
    if g1_setup is not None:
        d.kzg_load_setup_g1(g1_setup)
    return d


def on_a_fresh_context(g1_setup, call):
    d = kzg_device(g1_setup)
    try:
        return call(d)
    finally:
        d.close()


def small_polys(n):
    return [[(1000 * k + i) % 65537 for i in range(N)] for k in range(n)]


def test_calls_of_different_kinds_share_the_slab(sidecars, g1_setup):
    """1-blob verify, a synchronous signature call, 2 blob proofs, the 1-blob verify again: the
    slab moves and is rebound between them, and each result is that of a fresh context."""
    blobs, coms, proofs = (list(x) for x in zip(*sidecars))
    sk_be = [(i + 1).to_bytes(32, "big") for i in range(4)]
    msgs = [hashlib.sha256(b"helper-frame" + bytes([i])).digest() for i in range(4)]

    def verify_one(d):
        return d.kzg_verify_blob_proof_batch(blobs[:1], coms[:1], proofs[:1], each=True)

    def signatures(d):
        pks, sigs = d.sk_to_pk(sk_be), d.sign(sk_be, msgs)
        blob, offs = pack_blobs(sigs)
        bad = msgs[:3] + [bytes(32)]
        res = d.verify_requests(np.array([0, 3, 4], np.uint32), np.frombuffer(b"".join(pks), np.uint8), None,
                                np.frombuffer(b"".join(bad), np.uint8), blob, offs, bytes(32))
        return [bool(v) for v in res.valid]

    def prove_two(d):
        return d.kzg_blob_proofs(blobs[:2], coms[:2])

    want = [on_a_fresh_context(g1_setup, c) for c in (verify_one, signatures, prove_two)]
    assert want == [(True, [OK], [1]), [True, False], (proofs[:2], [OK, OK])]
    d = kzg_device(g1_setup)
    try:
        got = [c(d) for c in (verify_one, signatures, prove_two, verify_one)]
    finally:
        d.close()
    assert got == want + want[:1]


def test_per_item_verdicts_of_a_failed_batch_after_a_larger_call(sidecars):
    blobs, coms, proofs = (list(x) for x in zip(*sidecars))
    d = kzg_device(None)
    try:
        assert d.kzg_verify_blob_proof_batch(blobs, coms, proofs, each=True) == (True, [OK] * 3, [1] * 3)
        foreign = [proofs[0], proofs[2]]
        assert d.kzg_verify_blob_proof_batch(blobs[:2], coms[:2], foreign, each=True) == (False, [OK, OK], [1, 0])
    finally:
        d.close()


def test_msm_group_buffers_by_the_number_of_jobs(g1_setup):
    """One job first (the group buffers at their smallest), then a group and one more."""
    polys = small_polys(MSM_GROUP + 1)
    blobs = [K.blob_from_ints(f) for f in polys]
    want = [S.commit(f) for f in polys]
    d = kzg_device(g1_setup)
    try:
        assert d.kzg_blob_commitments(blobs[:1]) == (want[:1], [OK])
        assert d.kzg_blob_commitments(blobs) == (want, [OK] * len(polys))
    finally:
        d.close()


def test_stage_events_switched_off(sidecars, g1_setup):
    """The same results, and no stage is published by a shuffle, a KZG verify or a sampling."""
    blob, com, proof = sidecars[0]
    seed, active, inc = hashlib.sha256(b"helper-frame-stages").digest(), [0, 1, 2], [32, 1, 32]
    results = []
    for events in (True, False):
        d = kzg_device(None, stage_events=events)
        try:
            d.balance_table_put(inc)
            shuffled = d.index_list_shuffle(0, active, seed).tolist()
            stages = [[s for s, _ in d.last_stage_times()]]
            verdict = d.kzg_verify_blob_proof_batch([blob], [com], [proof], each=True)
            stages.append([s for s, _ in d.last_stage_times()])
            got = d.sample_by_balance([seed], 2, active, 32, 64)
            stages.append([s for s, _ in d.last_stage_times()])
            results.append((shuffled, verdict, got.indices.tolist(), got.found.tolist(), got.tried.tolist()))
        finally:
            d.close()
        assert stages == ([["shuffle"], ["kzg_hash", "kzg_eval", "kzg_tail"], ["sample"]] if events else [[], [], []])
    assert results[0] == results[1]
    assert results[0][0] == SH.unshuffle_spec(active, seed) and results[0][1] == (True, [OK], [1])
    want = SA.sample_rounds(seed, active, inc, 32, 2, 64)
    assert results[0][2:] == ([want[0]], [want[1]], [want[2]])
