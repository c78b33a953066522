"""lb_expand_set_keys, the expansion stage of lb_verify_requests_keys* alone, against the Python
expansion (tests/shuffle_helper.py expand_set_keys): the lengths around a lane's 64 bits and a
wave's 4,096, unaligned slices and bit offsets, the edge patterns, padding bits, mixed kinds."""
import numpy as np
import pytest

import shuffle_helper as SH
from lodestar_amd.native import LB_KEYS_BITS, LB_KEYS_DIRECT, LB_KEYS_SLICE, Device, LodestarBlsError

pytestmark = pytest.mark.gpu

LIST_N = 9000
LENS = [1, 63, 64, 65, 2048, 4097]


@pytest.fixture(scope="module")
def xdev():
    dev = Device(0)
    lists = {0: (np.arange(LIST_N, dtype=np.uint32) * 5 + 1), 3: np.array([7, 7, 1, 0, 99, 7] * 100, np.uint32)}
    for k, v in lists.items():
        dev.index_list_put(k, v)
    yield dev, lists
    dev.close()


def pack_bits(flags):
    """SSZ bit order: bit j = byte j // 8, bit j % 8"""
    return np.packbits(np.asarray(flags, np.uint8), bitorder="little").tobytes()


def check(dev, lists, sets, pool, bits):
    want_off, want_idx = SH.expand_set_keys(sets, pool, bits, lists)
    off, idx = dev.expand_set_keys(sets, pool, np.frombuffer(bits, np.uint8))
    assert np.array_equal(off, want_off)
    assert np.array_equal(idx, want_idx)
    return off, idx


def patterns(n, rnd):
    yield "zero", np.zeros(n, np.uint8)
    yield "one", np.ones(n, np.uint8)
    first = np.zeros(n, np.uint8)
    first[0] = 1
    yield "first", first
    last = np.zeros(n, np.uint8)
    last[n - 1] = 1
    yield "last", last
    yield "random", rnd.integers(0, 2, n).astype(np.uint8)


@pytest.mark.parametrize("n", LENS)
def test_bits_lengths_and_patterns(xdev, n):
    """One call holds every pattern of the length, each at an odd slice start and a bit offset
    that is no multiple of 4, the last byte's padding bits set."""
    dev, lists = xdev
    rnd = np.random.default_rng(n)
    sets, blob = [], bytearray(b"\xff" * 3)  # bits_off starts at 3
    for k, (_, flags) in enumerate(patterns(n, rnd)):
        raw = bytearray(pack_bits(flags))
        if n % 8:
            raw[-1] |= (0xFF << (n % 8)) & 0xFF  # padding bits: must be ignored
        sets.append((LB_KEYS_BITS, 0, 2 * k + 1, n, len(blob)))
        blob += raw
        while len(blob) % 2 == 0:  # every offset stays odd
            blob += b"\xff"
    assert all(s[4] % 4 for s in sets)
    off, _ = check(dev, lists, sets, None, bytes(blob))
    assert np.diff(off).tolist()[:4] == [0, n, 1, 1]


def test_mixed_kinds_in_one_call(xdev):
    dev, lists = xdev
    rnd = np.random.default_rng(7)
    pool = rnd.integers(0, 2 ** 32, 300, dtype=np.uint64).astype(np.uint32)
    f1, f2 = rnd.integers(0, 2, 130).astype(np.uint8), rnd.integers(0, 2, 600).astype(np.uint8)
    blob = b"\x00" + pack_bits(f1) + pack_bits(f2)
    sets = [(LB_KEYS_DIRECT, 0, 123456, 0, 0),
            (LB_KEYS_BITS, 0, 4001, 130, 1),
            (LB_KEYS_SLICE, 0, 17, 200, 0),
            (LB_KEYS_SLICE, 0, 5, 0, 0),           # an empty slice
            (LB_KEYS_BITS, 3, 0, 600, 1 + 17),     # a list with duplicates, the whole of it
            (LB_KEYS_DIRECT, 0, 0xFFFFFFFF, 0, 0),
            (LB_KEYS_SLICE, 0, 299, 1, 0),
            (LB_KEYS_BITS, 0, LIST_N - 5, 5, 2)]   # the list's last entries
    off, idx = check(dev, lists, sets, pool, blob)
    assert off[1] == 1 and idx[0] == 123456 and off[4] == off[3]
    # enough sets for several workgroups of four waves
    many = [sets[i % len(sets)] for i in range(37)]
    check(dev, lists, many, pool, blob)


def test_refusals(xdev):
    dev, lists = xdev
    ok = [(LB_KEYS_BITS, 0, 0, 16, 0)]
    assert dev.expand_set_keys(ok, None, b"\x01\x80")[1].tolist() == [1, 5 * 15 + 1]
    for bad, pool, bits in [
            ([(LB_KEYS_BITS, 1, 0, 16, 0)], None, b"\xff\xff"),            # an unloaded list
            ([(LB_KEYS_BITS, 8, 0, 16, 0)], None, b"\xff\xff"),            # no such list
            ([(LB_KEYS_BITS, 0, LIST_N - 15, 16, 0)], None, b"\xff\xff"),  # a + len beyond the list
            ([(LB_KEYS_BITS, 0, 0, 17, 0)], None, b"\xff\xff"),            # the bits' third byte is missing
            ([(LB_KEYS_BITS, 0, 0, 16, 1)], None, b"\xff\xff"),
            ([(LB_KEYS_SLICE, 0, 3, 2, 0)], np.arange(4, dtype=np.uint32), b""),  # beyond the pool
            ([(3, 0, 0, 1, 0)], None, b"\xff")]:                                    # an unknown kind
        with pytest.raises(LodestarBlsError):
            dev.expand_set_keys(ok + bad, pool, bits, max_indices=64)
    with pytest.raises(LodestarBlsError):  # more indices than the caller has room for
        dev.expand_set_keys(ok, None, b"\xff\xff", max_indices=15)
