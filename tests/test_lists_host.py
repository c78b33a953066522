"""Host-side packing of bits sets (no GPU): a package whose keys are all validator indices or
bits sets goes to the library as set descriptors (verify_requests_keys_async); one that holds a
key with bytes only falls back to today's form, its bits sets expanded from the device's list;
a package without bits sets is packed as it always was."""
import numpy as np
import pytest

from lodestar_amd.native import LB_KEYS_BITS, LB_KEYS_DIRECT, LB_KEYS_SLICE, SET_KEYS_DTYPE, Device, PendingCall, \
    VerifyResult
from lodestar_amd.verifier import BlsGpuVerifier, DeviceBackend, PublicKey, SignatureSetType, aggregate_set, bits_set, \
    pack_set_keys, single_set


class ListDev:
    """Stand-in for native.Device: records what a call ships."""

    def __init__(self):
        self.keys_calls, self.flat_calls, self.lists = [], [], {}

    def _pending(self, req_off, partial):
        n = len(req_off) - 1
        return PendingCall(1, n, 0, np.ones(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8), np.zeros(1, np.uint8),
                           None, partial)

    def verify_requests_keys_async(self, req_off, set_keys, pool, bits, msgs, blob, offs, seed, batchable=None,
                                   partial=False, priority=False):
        self.keys_calls.append((np.asarray(set_keys).tolist(), list(pool), bytes(bits), list(req_off)))
        return self._pending(req_off, partial)

    def verify_requests_async(self, req_off, pks, pk_off, msgs, blob, offs, seed, pk_indices=None, partial=False):
        self.flat_calls.append((pks, None if pk_indices is None else list(pk_indices), list(pk_off)))
        return self._pending(req_off, partial)

    def wait_call(self, pc):
        return VerifyResult(pc.valid[:pc.n_req], pc.err[:pc.n_req], np.zeros(0, np.uint8), 0.0)

    def index_list_put(self, list_id, indices):
        self.lists[list_id] = np.asarray(indices, np.uint32)

    def index_list_shuffle(self, list_id, active, seed):
        self.lists[list_id] = np.asarray(active, np.uint32)[::-1].copy()
        return self.lists[list_id]

    def index_list_read(self, list_id, first, n):
        return self.lists[list_id][first:first + n]

    def last_stage_times(self):
        return []

    def close(self):
        pass


ROOT, SIG = bytes(32), bytes(96)


def test_bits_set_constructor():
    s = bits_set(2, 64, 12, b"\x05\xf8\xff", ROOT, SIG)
    assert s.type == SignatureSetType.bits and (s.list_id, s.start, s.length) == (2, 64, 12)
    assert s.bits == b"\x05\xf8"  # ceil(12 / 8) bytes are kept
    with pytest.raises(ValueError):
        bits_set(0, 0, 17, b"\xff\xff", ROOT, SIG)


def test_descriptors_for_index_keys_and_bits_sets():
    b = DeviceBackend(seed_source=lambda: bytes(32), dev=ListDev())
    sets = [single_set(PublicKey(index=4), ROOT, SIG),
            bits_set(0, 32, 10, b"\x05\x02", ROOT, SIG),
            aggregate_set([PublicKey(index=9), PublicKey(index=8)], ROOT, SIG),
            bits_set(1, 0, 512, bytes(range(64)), ROOT, SIG),
            aggregate_set([], ROOT, SIG)]
    assert b.verify_requests([sets[:2], sets[2:]]) == ([True, True], [0, 0])
    rows, pool, bits, req_off = b.dev.keys_calls[-1]
    assert rows == [[LB_KEYS_DIRECT, 0, 4, 0, 0], [LB_KEYS_BITS, 0, 32, 10, 0], [LB_KEYS_SLICE, 0, 0, 2, 0],
                    [LB_KEYS_BITS, 1, 0, 512, 2], [LB_KEYS_SLICE, 0, 2, 0, 0]]
    assert pool == [9, 8] and bits == b"\x05\x02" + bytes(range(64)) and req_off == [0, 2, 5]
    assert b.dev.flat_calls == []
    b.close()


def test_fallback_for_a_key_with_bytes():
    b = DeviceBackend(seed_source=lambda: bytes(32), dev=ListDev())
    b.put_index_list(3, [70, 71, 72, 73, 74, 75, 76, 77, 78, 79])
    sets = [bits_set(3, 2, 6, b"\x29", ROOT, SIG),                      # bits 0, 3, 5 of entries 2..7
            single_set(PublicKey(bytes([7]) * 96), ROOT, SIG),
            single_set(PublicKey(index=5), ROOT, SIG)]
    assert pack_set_keys(sets) is None
    assert b.verify_requests([sets]) == ([True], [0])
    assert b.dev.keys_calls == []
    pks, idx, pk_off = b.dev.flat_calls[-1]
    assert idx == [72, 75, 77, 0x80000000, 5] and pk_off == [0, 3, 4, 5] and pks.tobytes() == bytes([7]) * 96
    b.close()


def test_packages_without_bits_sets_are_packed_as_before():
    b = DeviceBackend(seed_source=lambda: bytes(32), dev=ListDev())
    b.verify_requests([[single_set(PublicKey(index=4), ROOT, SIG),
                        aggregate_set([PublicKey(index=1), PublicKey(index=2)], ROOT, SIG)]])
    assert b.dev.keys_calls == []
    assert b.dev.flat_calls[-1] == (None, [4, 1, 2], [0, 1, 3])
    b.close()


def test_sync_shuffling_reaches_every_backend():
    backends = [DeviceBackend(seed_source=lambda: bytes(32), dev=ListDev()) for _ in range(2)]
    v = BlsGpuVerifier(backends=backends)
    out = v.sync_shuffling(1, [3, 4, 5], bytes(32))
    assert out.tolist() == [5, 4, 3]
    v.put_index_list(2, [9, 9])
    for b in backends:
        assert b.dev.lists[1].tolist() == [5, 4, 3] and b.dev.lists[2].tolist() == [9, 9]
        b.close()


def test_descriptor_rows_are_the_c_struct():
    """native packs rows of five u32 as lb_set_keys {kind, list, a, len, bits_off}: 20 bytes"""
    assert SET_KEYS_DTYPE.itemsize == 20 and SET_KEYS_DTYPE.names == ("kind", "list", "a", "len", "bits_off")
    ks, keep, n = Device._key_source([(2, 1, 32, 10, 7), (0, 0, 4, 0, 0)], [1, 2, 3], b"\x01\x02")
    assert n == 2 and (ks.n_pool, ks.n_bits_bytes) == (3, 2)
    assert keep[0].tobytes() == np.array([2, 1, 32, 10, 7, 0, 0, 4, 0, 0], "<u4").tobytes()
