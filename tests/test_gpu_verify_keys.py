"""lb_verify_requests_keys*: sets that name their keys by descriptor (a validator index, a slice
of explicit indices, bits over a slice of a device-resident index list) against the flat form
they expand to -- lb_verify_requests with pubkey_indices -- on every path the flat form has."""
import copy
import hashlib

import numpy as np
import pytest

import shuffle_helper as SH
from lodestar_amd.native import LB_KEYS_BITS, LB_KEYS_DIRECT, LB_KEYS_SLICE, LB_REQ_BAD_PUBKEY, \
    LB_REQ_EMPTY_AGGREGATE, Device, LodestarBlsError, pack_blobs
from oracle import bls12_381 as O

pytestmark = pytest.mark.gpu

N_KEYS = 300
SEED = hashlib.sha256(b"keys-seed").digest()


def sk_be(i):
    return O.interop_secret_key(i).to_bytes(32, "big")


def pack_bits(flags):
    return np.packbits(np.asarray(flags, np.uint8), bitorder="little").tobytes()


class Package:
    """Requests of sets given as descriptors, with the flat index form they expand to."""

    def __init__(self, dev, lists, reqs, pool, bits, tag):
        # reqs: [[descriptor, ...], ...]; one message per set, signed by the keys it expands to
        self.sets = [d for r in reqs for d in r]
        self.req_off = np.cumsum([0] + [len(r) for r in reqs]).astype(np.uint32)
        self.pool, self.bits = np.asarray(pool, np.uint32), bytes(bits)
        self.pk_off, self.idx = SH.expand_set_keys(self.sets, self.pool, self.bits, lists)
        ns = len(self.sets)
        self.msgs = [hashlib.sha256(tag + i.to_bytes(4, "little")).digest() for i in range(ns)]
        keys = [[int(v) for v in self.idx[self.pk_off[i]:self.pk_off[i + 1]]] for i in range(ns)]
        # (a set without keys, or with a key outside the table, keeps any well-formed signature)
        signers = [k if k and all(v < N_KEYS for v in k) else [0] for k in keys]
        parts = dev.sign([sk_be(v) for k in signers for v in k], [self.msgs[i] for i, k in enumerate(signers) for _ in k])
        at = np.cumsum([0] + [len(k) for k in signers])
        self.sigs, bad = dev.aggregate_signature_groups([parts[at[i]:at[i + 1]] for i in range(ns)])
        assert all(b == -1 for b in bad)

    def arrays(self):
        blob, offs = pack_blobs(self.sigs)
        return np.frombuffer(b"".join(self.msgs), np.uint8), blob, offs

    def by_keys(self, dev, **kw):
        msgs, blob, offs = self.arrays()
        fn = dev.verify_requests_keys_async if kw else dev.verify_requests_keys
        return fn(self.req_off, self.sets, self.pool, self.bits, msgs, blob, offs, SEED, **kw)

    def flat(self, dev, **kw):
        msgs, blob, offs = self.arrays()
        fn = dev.verify_requests_async if kw else dev.verify_requests
        return fn(self.req_off, None, self.pk_off, msgs, blob, offs, SEED, pk_indices=self.idx, **kw)


def same(a, b):
    assert a.valid.tolist() == b.valid.tolist()
    assert a.errors.tolist() == b.errors.tolist()
    assert a.set_status.tolist() == b.set_status.tolist()
    assert a.batch_retries == b.batch_retries


@pytest.fixture(scope="module")
def kdev():
    dev = Device(0)
    assert dev.pubkey_table_append(dev.sk_to_pk([sk_be(i) for i in range(N_KEYS)])) == N_KEYS
    rnd = np.random.default_rng(1)
    active = rnd.permutation(N_KEYS)[:128].astype(np.uint32)
    lists = {0: dev.index_list_shuffle(0, active, hashlib.sha256(b"epoch").digest()),
             1: rnd.integers(0, N_KEYS, 512).astype(np.uint32),   # a sync committee: duplicates
             2: np.array([3, N_KEYS + 4700, 5, 6], np.uint32)}    # an entry beyond the table
    assert np.array_equal(lists[0], SH.unshuffle_rounds(active, hashlib.sha256(b"epoch").digest()))
    assert len(set(lists[1].tolist())) < 512
    dev.index_list_put(1, lists[1])
    dev.index_list_put(2, lists[2])
    yield dev, lists
    dev.close()


def mixed_requests(rnd, n_req=40):
    """~40 requests of DIRECT, SLICE and BITS sets over the shuffling (committee slices of 32)
    and the 512-entry list"""
    pool, bits, reqs = [], bytearray(b"\x00"), []
    for _ in range(n_req):
        req = []
        for _ in range(int(rnd.choice([1, 1, 2, 3, 5]))):
            kind = int(rnd.choice([LB_KEYS_DIRECT, LB_KEYS_SLICE, LB_KEYS_BITS, LB_KEYS_BITS]))
            if kind == LB_KEYS_DIRECT:
                req.append((kind, 0, int(rnd.integers(0, N_KEYS)), 0, 0))
            elif kind == LB_KEYS_SLICE:
                n = int(rnd.integers(1, 20))
                req.append((kind, 0, len(pool), n, 0))
                pool += rnd.integers(0, N_KEYS, n).tolist()
            else:
                lid = int(rnd.integers(0, 2))
                if lid == 0:
                    start, n = 32 * int(rnd.integers(0, 4)), 32
                else:
                    n = int(rnd.integers(1, 130))
                    start = int(rnd.integers(0, 512 - n))
                flags = rnd.integers(0, 2, n).astype(np.uint8)
                flags[int(rnd.integers(0, n))] = 1
                req.append((kind, lid, start, n, len(bits)))
                bits += pack_bits(flags)
        reqs.append(req)
    return reqs, pool, bits


@pytest.fixture(scope="module")
def packages(kdev):
    dev, lists = kdev
    reqs, pool, bits = mixed_requests(np.random.default_rng(2))
    good = Package(dev, lists, reqs, pool, bits, b"pkg")
    bad = copy.copy(good)
    s = int(bad.req_off[17])
    bad.sigs = list(good.sigs)
    bad.sigs[s] = good.sigs[s + 1 if bad.req_off[18] - s > 1 else s - 1]  # a valid point, the wrong signature
    assert {d[0] for d in good.sets} == {LB_KEYS_DIRECT, LB_KEYS_SLICE, LB_KEYS_BITS}
    return good, bad


@pytest.mark.parametrize("lp_max", [1024, 0], ids=["latency_path", "pipeline"])
def test_parity_with_the_flat_form(kdev, packages, lp_max):
    dev, _ = kdev
    good, bad = packages
    dev.set_latency_path(lp_max)
    try:
        for p, expect in ((bad, [k != 17 for k in range(40)]), (good, [True] * 40)):
            by_keys = p.by_keys(dev)
            stages = [s for s, _ in dev.last_stage_times()]
            assert stages[0] == "expand_keys" and ("lp_verify" in stages) == (lp_max != 0)
            flat = p.flat(dev)
            assert [s for s, _ in dev.last_stage_times()] == stages[1:]  # the same call behind the expansion
            same(by_keys, flat)
            assert [bool(v) for v in by_keys.valid] == expect
    finally:
        dev.set_latency_path(1024)


def test_bits_matter(kdev):
    dev, lists = kdev
    flags = np.zeros(32, np.uint8)
    flags[[1, 4, 9, 30]] = 1
    good = Package(dev, lists, [[(LB_KEYS_BITS, 0, 64, 32, 0)]], [], pack_bits(flags), b"bits")
    assert good.by_keys(dev).valid.tolist() == [1]
    for flip in (9, 10):  # a participant cleared, a non-participant set
        f2 = flags.copy()
        f2[flip] ^= 1
        good.bits = pack_bits(f2)
        res = good.by_keys(dev)
        assert res.valid.tolist() == [0] and res.errors.tolist() == [0]
    # the same bits over another slice of the list: other keys
    good.bits = pack_bits(flags)
    good.sets = [(LB_KEYS_BITS, 0, 32, 32, 0)]
    assert good.by_keys(dev).valid.tolist() == [0]


def test_edge_verdicts(kdev):
    dev, lists = kdev
    reqs = [[(LB_KEYS_DIRECT, 0, 7, 0, 0)],
            [(LB_KEYS_DIRECT, 0, 8, 0, 0), (LB_KEYS_BITS, 0, 0, 32, 0)],    # no bit set
            [(LB_KEYS_SLICE, 0, 0, 0, 0)],                                   # an empty slice
            [(LB_KEYS_BITS, 2, 0, 4, 4)],                                    # bits 0, 1: entry 1 is beyond the table
            [(LB_KEYS_BITS, 2, 0, 4, 5)],                                    # bits 0, 2, 3 (padding bits set): fine
            [(LB_KEYS_DIRECT, 0, N_KEYS, 0, 0)]]                             # the first index beyond the table
    p = Package(dev, lists, reqs, [], bytes(4) + b"\x03\xfd", b"edge")
    res, flat = p.by_keys(dev), p.flat(dev)
    same(res, flat)
    assert res.valid.tolist() == [1, 0, 0, 0, 1, 0]
    assert res.errors.tolist() == [0, LB_REQ_EMPTY_AGGREGATE, LB_REQ_EMPTY_AGGREGATE, LB_REQ_BAD_PUBKEY, 0,
                                   LB_REQ_BAD_PUBKEY]


def test_submit_time_refusals_enqueue_nothing(kdev):
    dev, lists = kdev
    ok = [(LB_KEYS_DIRECT, 0, 7, 0, 0)]
    p = Package(dev, lists, [ok, [(LB_KEYS_BITS, 0, 0, 8, 0)]], [], b"\x11", b"refuse")
    assert p.by_keys(dev).valid.tolist() == [1, 1]
    for bad in [(LB_KEYS_BITS, 5, 0, 8, 0),      # an unloaded list
                (LB_KEYS_BITS, 0, 121, 8, 0),    # a + len beyond the 128-entry list
                (LB_KEYS_BITS, 0, 0, 9, 0),      # bits_off + ceil(len / 8) beyond n_bits_bytes
                (LB_KEYS_SLICE, 0, 0, 1, 0),     # beyond the (empty) pool
                (9, 0, 0, 0, 0)]:                # an unknown kind
        p.sets = ok + [bad]
        for kw in ({}, {"priority": True}, {"partial": True}, {"partial": False}):
            with pytest.raises(LodestarBlsError, match="lb_key_source: set 1"):
                p.by_keys(dev, **kw)
    # nothing is in flight, and the context serves the next call
    p.sets = ok + [(LB_KEYS_BITS, 0, 0, 8, 0)]
    assert p.by_keys(dev).valid.tolist() == [1, 1]


def test_async_priority_and_two_phase(kdev, packages):
    dev, _ = kdev
    good, bad = packages
    want_good, want_bad = good.flat(dev), bad.flat(dev)
    # three calls in flight
    calls = [p.by_keys(dev, partial=False) for p in (good, bad, good)]
    for pc, want in zip(calls, (want_good, want_bad, want_good)):
        res = dev.wait_call(pc)
        assert res.valid.tolist() == want.valid.tolist() and res.errors.tolist() == want.errors.tolist()
    # the priority lane
    res = dev.wait_call(bad.by_keys(dev, priority=True))
    assert res.valid.tolist() == want_bad.valid.tolist() and res.set_status.tolist() == want_bad.set_status.tolist()
    # two-phase: the partial, the host's check, the verdict
    for p, want, ok in ((good, want_good, True), (bad, want_bad, False)):
        got = []
        for pc in (p.by_keys(dev, partial=True), p.flat(dev, partial=True)):
            assert dev.gt_check([dev.partial_wait(pc)]) is ok
            dev.verify_finish(pc, ok)
            got.append(dev.wait_call(pc))
        same(got[0], got[1])
        assert got[0].valid.tolist() == want.valid.tolist() and got[0].errors.tolist() == want.errors.tolist()
