"""Balance-weighted sampling off the GPU: the two hashlib restatements of lb_sample_by_balance's
walk agree (tests/sample_helper.py); the cases tests/test_gpu_sample.py runs have, for the
restatement, the properties that test relies on, so none of them is vacuous; and the Python
hosts ship what computeProposers / getNextSyncCommittee need, over a stand-in device."""
import hashlib

import numpy as np
import pytest

import sample_helper as SA
from lodestar_amd import native
from lodestar_amd.native import LB_NO_LIST, LB_SAMPLE_NONE, SampleResult, sample_first_pass
from lodestar_amd.verifier import BlsGpuVerifier, DeviceBackend


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_restatements_agree(n):
    rnd = np.random.default_rng(n)
    seed = rnd.bytes(32)
    active = rnd.permutation(2 * n)[:n].astype(np.uint32)
    inc = rnd.integers(0, 33, 2 * n).astype(np.uint8)
    for count, cap in ((1, n), (7, 200), (7, 3)):
        assert SA.sample_spec(seed, active, inc, 32, count, cap) == SA.sample_rounds(seed, active, inc, 32, count, cap)


def test_size_cases_cross_the_second_counter_byte():
    """tried > 8,192: LE64(i div 32) takes a second byte; n < 512 wraps and repeats"""
    for n in SA.SIZES:
        out, found, tried = SA.sample_rounds(*SA.size_case(n))
        assert found == 512 and 8192 < tried < (1 << 20)
        if n < 512:
            assert tried > n and len(set(out)) < 512


def test_passes_case_needs_more_than_three_passes():
    out, found, tried = SA.sample_rounds(*SA.passes_case())
    first = sample_first_pass(512)
    assert first == 1024 and sample_first_pass(1) == 64 and sample_first_pass(33) == 128
    assert found == 512 and tried > first + 2 * first + 4 * first


def test_proposers_case_exercises_rejection():
    epoch_seed, start, active, inc = SA.proposers_case()
    tried = [SA.sample_rounds(s, active, inc, 32, 1, len(active))[2] for s in SA.slot_seeds(epoch_seed, start)]
    assert {3, 4, 5} <= set(tried)


def test_unfilled_case_fills_exactly_one_seed():
    seeds, active, inc = SA.unfilled_case()
    res = [SA.sample_spec(s, active, inc, 32, 1, 3) for s in seeds]
    assert sum(f for _, f, _ in res) == 1
    assert all((o, t) == ([SA.NONE], 3) for o, f, t in res if f == 0)


def test_range_case_has_products_of_sixteen_bits():
    seed, active, inc, max_inc, count, cap = SA.range_case()
    assert max_inc == 255 and int(inc[active].max()) * 255 >= 1 << 15  # the sixteenth bit
    assert SA.sample_rounds(seed, active, inc, max_inc, count, cap)[1] == count


def test_constants_are_the_header_s():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "lodestar_bls.h")).read()
    for name in ("LB_SAMPLE_MAX_SEEDS", "LB_SAMPLE_MAX_COUNT", "LB_SAMPLE_MAX_CANDIDATES", "LB_SAMPLE_NONE",
                 "LB_NO_LIST", "LB_SAMPLE_PASS_MAX"):
        m = re.search(r"#define %s (\w+?)u\b" % name, hdr)
        assert m and int(m.group(1), 0) == getattr(native, name), name


class SampleDev:
    """Stand-in for native.Device: records what a call ships."""

    def __init__(self, found=None):
        self.samples, self.balances, self.aggs, self.found = [], [], [], found

    def balance_table_put(self, increments, first=0):
        self.balances.append((bytes(increments), first))
        return first + len(increments)

    def sample_by_balance(self, seeds, count, active_indices, max_increment, max_candidates, store_list=LB_NO_LIST):
        self.samples.append((list(seeds), count, list(active_indices), max_increment, max_candidates, store_list))
        ns = len(seeds)
        out = np.arange(ns * count, dtype=np.uint32).reshape(ns, count) + 100
        out[1::2] = LB_SAMPLE_NONE
        found = np.full(ns, count if self.found is None else self.found, np.uint32)
        return SampleResult(out, found, np.ones(ns, np.uint32))

    def aggregate_pubkeys_list(self, list_id, first, n):
        self.aggs.append((list_id, first, n))
        return bytes([list_id]) * 96

    def close(self):
        pass


def test_compute_proposers_ships_the_slot_seeds():
    b = DeviceBackend(seed_source=lambda: bytes(32), dev=SampleDev())
    epoch_seed = bytes(range(32))
    got = b.compute_proposers(epoch_seed, 64, [9, 8, 7, 6, 5])
    seeds, count, active, max_inc, cap, store = b.dev.samples[-1]
    assert seeds == [hashlib.sha256(epoch_seed + (64 + i).to_bytes(8, "little")).digest() for i in range(32)]
    assert (count, active, max_inc, cap, store) == (1, [9, 8, 7, 6, 5], 32, 5, LB_NO_LIST)
    assert got == [100 + i if i % 2 == 0 else -1 for i in range(32)]  # LB_SAMPLE_NONE -> -1
    assert len(b.compute_proposers(epoch_seed, 0, [1, 2], slots=4)) == 4
    b.close()


def test_sync_committee_stores_the_list_and_raises_when_unfilled():
    b = DeviceBackend(seed_source=lambda: bytes(32), dev=SampleDev())
    idx, agg = b.sync_committee(5, [4, 5, 6], bytes([3]) * 32)
    assert b.dev.samples[-1] == ([bytes([3]) * 32], 512, [4, 5, 6], 32, native.LB_SAMPLE_MAX_CANDIDATES, 5)
    assert idx.tolist() == list(range(100, 612)) and agg == bytes([5]) * 96 and b.dev.aggs == [(5, 0, 512)]
    b.close()
    b = DeviceBackend(seed_source=lambda: bytes(32), dev=SampleDev(found=511))
    with pytest.raises(RuntimeError, match="not filled"):
        b.sync_committee(5, [4, 5, 6], bytes(32), max_candidates=1000)
    assert b.dev.aggs == []
    b.close()


def test_sync_balances_forwards_first_to_every_backend():
    backends = [DeviceBackend(seed_source=lambda: bytes(32), dev=SampleDev()) for _ in range(2)]
    v = BlsGpuVerifier(backends=backends)
    assert v.sync_balances(bytes([32, 31, 0]), first=7) == 10
    assert v.compute_proposers(bytes(32), 0, [1, 2, 3], slots=2) == [100, -1]
    idx, agg = v.sync_committee(2, [1, 2, 3], bytes(32), size=4)
    assert idx.tolist() == [100, 101, 102, 103] and agg == bytes([2]) * 96
    for b in backends:
        assert b.dev.balances == [(bytes([32, 31, 0]), 7)]
        assert b.dev.samples[-1][1:] == (4, [1, 2, 3], 32, native.LB_SAMPLE_MAX_CANDIDATES, 2)
        b.close()
    assert len(backends[0].dev.samples) == 2 and len(backends[1].dev.samples) == 1  # proposers: one GPU
