"""Device-resident index lists: lb_index_list_shuffle against the reference's unshuffleList
vectors and the hashlib restatements (tests/shuffle_helper.py), at the sizes where the kernels
take another step -- one digest, the 256-position boundary, a second byte of the digest index --
and lb_index_list_put / _size / _read with their refusals."""
import hashlib

import numpy as np
import pytest

import shuffle_helper as SH
from lodestar_amd.native import LB_INDEX_LISTS, LB_SHUFFLE_MAX, Device, LodestarBlsError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ldev():
    dev = Device(0)
    yield dev
    dev.close()


def test_shuffle_kat(ldev):
    seed, cases = SH.load_kat()
    for inp, res in cases:
        assert ldev.index_list_shuffle(0, inp, seed).tolist() == res
        assert ldev.index_list_size(0) == len(inp)
        assert ldev.index_list_read(0, 0, len(inp)).tolist() == res


@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 511, 513, 65537])
def test_shuffle_matches_helper(ldev, n):
    seed = hashlib.sha256(b"gpu-shuffle" + n.to_bytes(4, "little")).digest()
    active = np.arange(n, dtype=np.uint32)
    got = ldev.index_list_shuffle(1, active, seed)
    assert np.array_equal(got, SH.unshuffle_rounds(active, seed))
    # out_shuffling is the stored list
    assert np.array_equal(ldev.index_list_read(1, 0, n), got)
    # (n <= 1 is a plain upload: no shuffle stage)
    assert [s for s, _ in ldev.last_stage_times()] == (["shuffle"] if n > 1 else [])


def test_shuffle_of_duplicate_carrying_indices(ldev):
    rnd = np.random.default_rng(20261020)
    n = 1000
    active = rnd.integers(0, 700, n).astype(np.uint32) * 3 + 11  # duplicates, not the identity
    seed = rnd.bytes(32)
    got = ldev.index_list_shuffle(2, active, seed)
    assert np.array_equal(got, SH.unshuffle_rounds(active, seed))
    assert ldev.index_list_shuffle(2, active, seed, want_output=False) is None  # out_shuffling is optional
    assert np.array_equal(ldev.index_list_read(2, 0, n), got)


def test_second_list_leaves_the_first_intact(ldev):
    seed_a, seed_b = bytes([1]) * 32, bytes([2]) * 32
    a = ldev.index_list_shuffle(3, np.arange(300, dtype=np.uint32), seed_a)
    b = ldev.index_list_shuffle(4, np.arange(5000, dtype=np.uint32) + 7, seed_b)  # (a new allocation)
    assert not np.array_equal(a, b[:300])
    assert np.array_equal(ldev.index_list_read(3, 0, 300), a)
    assert np.array_equal(ldev.index_list_read(4, 4990, 10), b[4990:])
    assert (ldev.index_list_size(3), ldev.index_list_size(4)) == (300, 5000)


def test_put_read_and_empty(ldev):
    sync = np.array([5, 9, 9, 0, 4000000000, 5] * 85 + [1, 2], np.uint32)  # 512, duplicates kept
    ldev.index_list_put(5, sync)
    assert ldev.index_list_size(5) == 512
    assert np.array_equal(ldev.index_list_read(5, 0, 512), sync)
    assert np.array_equal(ldev.index_list_read(5, 500, 12), sync[500:])
    assert len(ldev.index_list_read(5, 512, 0)) == 0
    ldev.index_list_put(5, [])
    assert ldev.index_list_size(5) == 0
    assert ldev.index_list_size(7) == 0  # never loaded


def test_refusals_change_nothing(ldev):
    keep = ldev.index_list_shuffle(6, np.arange(40, dtype=np.uint32), bytes(32))
    with pytest.raises(LodestarBlsError):  # above the cap: refused before anything is read
        big = np.zeros(LB_SHUFFLE_MAX + 1, np.uint32)
        ldev.index_list_shuffle(6, big, bytes(32))
    with pytest.raises(LodestarBlsError):
        ldev.index_list_shuffle(LB_INDEX_LISTS, np.arange(4, dtype=np.uint32), bytes(32))
    with pytest.raises(LodestarBlsError):
        ldev.index_list_put(LB_INDEX_LISTS, [1, 2])
    with pytest.raises(LodestarBlsError):
        ldev.index_list_size(LB_INDEX_LISTS)
    with pytest.raises(LodestarBlsError):
        ldev.index_list_read(6, 30, 11)  # one past the end
    with pytest.raises(LodestarBlsError):
        ldev.index_list_read(LB_INDEX_LISTS, 0, 1)
    assert ldev.index_list_size(6) == 40
    assert np.array_equal(ldev.index_list_read(6, 0, 40), keep)
