"""lb_sample_by_balance, lb_balance_table_* and lb_aggregate_pubkeys_list against the hashlib
restatements of tests/sample_helper.py, every comparison exact: the sizes where the shuffle
crosses a digest and a digest-index byte and the walk's counter takes a second byte, several
passes, proposers (32 seeds, one place each), seeds that do not fill, the 16-bit product, the
list stored on the device, and the refusals, which change nothing.
tests/test_sample_host.py checks on the CPU that each case has the property it is here for."""
import numpy as np
import pytest

import sample_helper as SA
import shuffle_helper as SH
from lodestar_amd.native import (LB_INDEX_LISTS, LB_KEYS_BITS, LB_NO_LIST, LB_SAMPLE_MAX_CANDIDATES,
                                 LB_SAMPLE_MAX_COUNT, LB_SAMPLE_MAX_SEEDS, LB_SAMPLE_NONE, LB_SHUFFLE_MAX,
                                 BadPubkeyError, Device, LodestarBlsError, sample_first_pass)
from lodestar_amd.verifier import DeviceBackend

pytestmark = pytest.mark.gpu

N_KEYS = 300


@pytest.fixture(scope="module")
def sdev():
    dev = Device(0)
    dev.pubkey_table_append(dev.sk_to_pk([(i + 1).to_bytes(32, "big") for i in range(N_KEYS)]))
    yield dev
    dev.close()


def check(dev, seeds, active, inc, max_inc, count, cap, store_list=LB_NO_LIST):
    """One call against sample_rounds per seed; -> the SampleResult"""
    dev.balance_table_put(inc)
    got = dev.sample_by_balance(seeds, count, active, max_inc, cap, store_list=store_list)
    want = [SA.sample_rounds(s, active, inc, max_inc, count, cap) for s in seeds]
    assert got.indices.tolist() == [w[0] for w in want]
    assert got.found.tolist() == [w[1] for w in want]
    assert got.tried.tolist() == [w[2] for w in want]
    assert [s for s, _ in dev.last_stage_times()] == ["sample"]
    return got


@pytest.mark.parametrize("n", SA.SIZES)
def test_sizes(sdev, n):
    seed, active, inc, max_inc, count, cap = SA.size_case(n)
    got = check(sdev, [seed], active, inc, max_inc, count, cap)
    assert got.found[0] == count and got.tried[0] > 8192


def test_several_passes(sdev):
    seed, active, inc, max_inc, count, cap = SA.passes_case()
    got = check(sdev, [seed], active, inc, max_inc, count, cap)
    first = sample_first_pass(count)
    assert got.tried[0] > first + 2 * first + 4 * first  # beyond the third pass


def test_proposers(sdev):
    epoch_seed, start, active, inc = SA.proposers_case()
    got = check(sdev, SA.slot_seeds(epoch_seed, start), active, inc, 32, 1, len(active))
    assert {3, 4, 5} <= set(got.tried.tolist())


def test_unfilled_seeds_and_zero_increments(sdev):
    seeds, active, inc = SA.unfilled_case()
    got = check(sdev, seeds, active, inc, 32, 1, 3)
    assert int(got.found.sum()) == 1
    for s in range(64):
        if got.found[s] == 0:
            assert (got.indices[s, 0], got.tried[s]) == (LB_SAMPLE_NONE, 3)
    # a committee that fills only in part: the places behind `found` stay LB_SAMPLE_NONE
    part = check(sdev, seeds[:2], np.arange(40, dtype=np.uint32), np.ones(40, np.uint8), 32, 16, 100)
    f = int(part.found[0])
    assert 0 < f < 16 and part.indices[0, f:].tolist() == [LB_SAMPLE_NONE] * (16 - f)


def test_products_of_sixteen_bits(sdev):
    seed, active, inc, max_inc, count, cap = SA.range_case()
    check(sdev, [seed, bytes(32)], active, inc, max_inc, count, cap)


def test_store_list(sdev):
    seed, active, inc, max_inc, count, cap = SA.size_case(257)
    got = check(sdev, [seed], active, inc, max_inc, count, cap, store_list=6)
    assert sdev.index_list_size(6) == count
    stored = sdev.index_list_read(6, 0, count)
    assert np.array_equal(stored, got.indices[0])
    rnd = np.random.default_rng(6)
    bits = np.packbits(rnd.integers(0, 2, 500).astype(np.uint8), bitorder="little").tobytes()
    sets = [(LB_KEYS_BITS, 6, 7, 500, 0)]
    want_off, want_idx = SH.expand_set_keys(sets, None, bits, {6: stored})
    off, idx = sdev.expand_set_keys(sets, None, np.frombuffer(bits, np.uint8))
    assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx)
    # a seed that does not fill leaves the list's content and size
    un = check(sdev, [seed], active, inc, max_inc, count, 9000, store_list=6)
    assert un.found[0] < count
    assert sdev.index_list_size(6) == count and np.array_equal(sdev.index_list_read(6, 0, count), stored)
    # a shorter committee replaces it
    short = check(sdev, [seed], active, inc, max_inc, 5, cap, store_list=6)
    assert sdev.index_list_size(6) == 5 and np.array_equal(sdev.index_list_read(6, 0, 5), short.indices[0])


def test_refusals_change_nothing(sdev):
    seed, active, inc, max_inc, count, cap = SA.size_case(257)
    keep = check(sdev, [seed], active, inc, max_inc, 8, cap, store_list=5).indices[0].copy()
    size = sdev.balance_table_size()
    beyond = active.copy()
    beyond[-1] = size  # examined or not, an index outside the table refuses the call
    seeds2 = [seed, bytes(32)]
    for seeds, cnt, act, mi, mc, store in [
            ([seed], 8, np.zeros(0, np.uint32), 32, 100, 5),                    # n == 0
            ([seed], 0, active, 32, 100, 5),                                     # count == 0
            ([seed], LB_SAMPLE_MAX_COUNT + 1, active, 32, 100, 5),
            ([seed] * (LB_SAMPLE_MAX_SEEDS + 1), 1, active, 32, 100, LB_NO_LIST),
            ([seed], 8, np.zeros(LB_SHUFFLE_MAX + 1, np.uint32), 32, 100, 5),
            ([seed], 8, active, 32, LB_SAMPLE_MAX_CANDIDATES + 1, 5),
            ([seed], 8, active, 32, 0, 5),
            ([seed], 8, active, 0, 100, 5),                                      # max_increment == 0
            ([seed], 8, active, 256, 100, 5),
            (seeds2, 8, active, 32, 100, 5),                                     # a list id with two seeds
            ([seed], 8, active, 32, 100, LB_INDEX_LISTS),                        # no such list
            ([seed], 8, beyond, 32, cap, 5)]:
        out = tuple(np.full(max(len(seeds) * cnt, 1), 0xA5A5A5A5, np.uint32) for _ in range(3))  # a sentinel
        with pytest.raises(LodestarBlsError):
            sdev.sample_by_balance(seeds, cnt, act, mi, mc, store_list=store, out=out)
        for arr in out:
            assert (arr == 0xA5A5A5A5).all()
        assert sdev.index_list_size(5) == 8 and np.array_equal(sdev.index_list_read(5, 0, 8), keep)
    # no seeds: nothing to do, nothing written
    out = tuple(np.full(8, 0xA5A5A5A5, np.uint32) for _ in range(3))
    none = sdev.sample_by_balance([], 8, active, 32, 100, out=out)
    assert none.indices.shape == (0, 8) and all((a == 0xA5A5A5A5).all() for a in out)


def test_balance_table():
    dev = Device(0)
    try:
        assert dev.balance_table_size() == 0
        a = (np.arange(5000) % 33).astype(np.uint8)
        assert dev.balance_table_put(a) == 5000
        assert np.array_equal(dev.balance_table_read(0, 5000), a)
        assert dev.balance_table_put(bytes([200, 201, 202]), first=1000) == 5000  # an inner range
        a[1000:1003] = [200, 201, 202]
        b = np.full(4000, 7, np.uint8)
        assert dev.balance_table_put(b, first=4990) == 8990  # overwrite the tail and append (the table grows)
        want = np.concatenate([a[:4990], b])
        assert np.array_equal(dev.balance_table_read(0, 8990), want)
        assert np.array_equal(dev.balance_table_read(4980, 20), want[4980:5000])
        assert dev.balance_table_put(bytes([9]), first=8990) == 8991  # first == size appends
        with pytest.raises(LodestarBlsError):
            dev.balance_table_put(bytes([1]), first=8992)  # a gap
        with pytest.raises(LodestarBlsError):
            dev.balance_table_read(8990, 2)
        assert dev.balance_table_size() == 8991 and dev.balance_table_read(8990, 1)[0] == 9
    finally:
        dev.close()


def test_aggregate_pubkeys_list(sdev):
    seed = bytes([8]) * 32
    active = np.arange(200, dtype=np.uint32) + 50  # n < 512: the committee repeats validators
    sdev.balance_table_put(np.full(250, 32, np.uint8))
    got = sdev.sample_by_balance([seed], 512, active, 32, 1 << 16, store_list=4)
    idx = sdev.index_list_read(4, 0, 512)
    assert got.found[0] == 512 and len(set(idx.tolist())) < 512 and np.array_equal(idx, got.indices[0])
    assert sdev.aggregate_pubkeys_list(4, 0, 512) == sdev.aggregate_pubkeys_indexed(idx)
    assert sdev.aggregate_pubkeys_list(4, 129, 67) == sdev.aggregate_pubkeys_indexed(idx[129:196])
    assert sdev.aggregate_pubkeys_list(4, 511, 1) == sdev.pubkey_table_read(int(idx[511]), 1)[0]
    for first, n in ((0, 0), (0, 513), (512, 1), (500, 13)):
        with pytest.raises(LodestarBlsError):
            sdev.aggregate_pubkeys_list(4, first, n)
    with pytest.raises(LodestarBlsError):
        sdev.aggregate_pubkeys_list(LB_INDEX_LISTS, 0, 1)
    with pytest.raises(LodestarBlsError):
        sdev.aggregate_pubkeys_list(7, 0, 1)  # never loaded
    sdev.index_list_put(3, [1, 2, N_KEYS, 3])  # an entry beyond the pubkey table
    with pytest.raises(BadPubkeyError, match="BAD_ENCODING"):
        sdev.aggregate_pubkeys_list(3, 0, 4)
    assert sdev.aggregate_pubkeys_list(3, 0, 2) == sdev.aggregate_pubkeys_indexed([1, 2])


def test_hosts_through_device_backend():
    b = DeviceBackend(0)
    try:
        b.sync_pubkeys(b.dev.sk_to_pk([(i + 1).to_bytes(32, "big") for i in range(N_KEYS)]))
        epoch_seed, start, active, inc = SA.proposers_case()
        active = active[:N_KEYS - 5]
        assert b.sync_balances(inc) == len(inc)
        want = [SA.sample_rounds(s, active, inc, 32, 1, len(active))[0][0] for s in SA.slot_seeds(epoch_seed, start)]
        assert b.compute_proposers(epoch_seed, start, active) == [-1 if w == SA.NONE else w for w in want]
        assert b.compute_proposers(epoch_seed, start, active[:1], slots=3, max_increment=255) == [
            (-1 if w == SA.NONE else w) for w in
            (SA.sample_spec(s, active[:1], inc, 255, 1, 1)[0][0] for s in SA.slot_seeds(epoch_seed, start, 3))]
        seed = bytes([5]) * 32
        idx, agg = b.sync_committee(2, active, seed)
        assert idx.tolist() == SA.sample_rounds(seed, active, inc, 32, 512, LB_SAMPLE_MAX_CANDIDATES)[0]
        assert agg == b.dev.aggregate_pubkeys_indexed(idx)
        assert np.array_equal(b.dev.index_list_read(2, 0, 512), idx)
        with pytest.raises(RuntimeError, match="not filled"):
            b.sync_committee(2, active, seed, max_candidates=600)
        assert np.array_equal(b.dev.index_list_read(2, 0, 512), idx)
    finally:
        b.close()
