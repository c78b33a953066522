"""Two restatements of the consensus spec's swap-or-not shuffle with hashlib, the reference of
lb_index_list_shuffle's tests:

    unshuffle_spec(active, seed)    out[i] = active[compute_shuffled_index(i, n, seed)], the spec's
                                    per-index form (phase0 beacon-chain.md compute_shuffled_index)
    unshuffle_rounds(active, seed)  the same permutation a round at a time over every position
                                    with numpy, for the larger sizes

which is what unshuffleList(activeIndices, seed) (state-transition/src/util/shuffle.ts) leaves in
its input and computeEpochShuffling (util/epochShuffling.ts:62-101) slices its committees from."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

SHUFFLE_ROUND_COUNT = 90
KAT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shuffle_kat.json")


def load_kat():
    """(seed, [(input, expected), ...]) of tests/golden/shuffle_kat.json"""
    with open(KAT_PATH) as f:
        kat = json.load(f)
    return bytes(kat["seed"]), [(list(c["input"]), list(c["res"])) for c in kat["cases"]]


def compute_shuffled_index(index: int, n: int, seed: bytes) -> int:
    assert 0 <= index < n and len(seed) == 32
    for r in range(SHUFFLE_ROUND_COUNT):
        rb = bytes([r])
        pivot = int.from_bytes(hashlib.sha256(seed + rb).digest()[:8], "little") % n
        flip = (pivot + n - index) % n
        position = max(index, flip)
        source = hashlib.sha256(seed + rb + (position // 256).to_bytes(4, "little")).digest()
        byte = source[(position % 256) // 8]
        if (byte >> (position % 8)) & 1:
            index = flip
    return index


def unshuffle_spec(active, seed: bytes):
    n = len(active)
    return [active[compute_shuffled_index(i, n, seed)] for i in range(n)]


def unshuffle_rounds(active, seed: bytes) -> np.ndarray:
    active = np.asarray(active, dtype=np.uint32)
    n = len(active)
    if n <= 1:
        return active.copy()
    idx = np.arange(n, dtype=np.int64)
    nblk = (n + 255) // 256
    for r in range(SHUFFLE_ROUND_COUNT):
        rb = bytes([r])
        pivot = int.from_bytes(hashlib.sha256(seed + rb).digest()[:8], "little") % n
        row = np.frombuffer(b"".join(hashlib.sha256(seed + rb + k.to_bytes(4, "little")).digest()
                                     for k in range(nblk)), dtype=np.uint8)
        flip = (pivot + n - idx) % n
        pos = np.maximum(idx, flip)
        bit = (row[pos >> 3] >> (pos & 7).astype(np.uint8)) & 1
        idx = np.where(bit == 1, flip, idx)
    return active[idx]


def expand_set_keys(set_keys, key_pool, bits, lists):
    """The Python expansion of lb_set_keys descriptors (kind, list, a, len, bits_off) ->
    (pk_offsets, indices): DIRECT a; SLICE key_pool[a : a + len]; BITS lists[list][a + j] for
    every j < len with bit j of bits[bits_off ..] set (bit j = byte j // 8, bit j % 8)."""
    off, out = [0], []
    for kind, lid, a, ln, bo in set_keys:
        kind, lid, a, ln, bo = int(kind), int(lid), int(a), int(ln), int(bo)
        if kind == 0:
            out.append(a)
        elif kind == 1:
            out.extend(int(v) for v in key_pool[a:a + ln])
        elif kind == 2:
            out.extend(int(lists[lid][a + j]) for j in range(ln) if (bits[bo + j // 8] >> (j % 8)) & 1)
        else:
            raise ValueError("unknown kind %d" % kind)
        off.append(len(out))
    return np.array(off, np.uint32), np.array(out, np.uint32)
