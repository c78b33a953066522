"""Two restatements, with hashlib, of the balance-weighted sampling include/lodestar_bls.h states
above lb_sample_by_balance -- computeProposerIndex and getNextSyncCommitteeIndices of the
reference (state-transition/src/util/seed.ts:22-80, 92-126) with the walk bounded:

    sample_spec(...)    every candidate through shuffle_helper.compute_shuffled_index
    sample_rounds(...)  candidates taken from shuffle_helper.unshuffle_rounds(active, seed)[i % n],
                        the whole permutation once, for the larger sizes

Both return (indices[count] with NONE where unfilled, found, tried)."""
from __future__ import annotations

import hashlib

import numpy as np

import shuffle_helper as SH

NONE = 0xFFFFFFFF


def _walk(cand_at, n, seed, inc, max_inc, count, max_candidates):
    out, tried, digest, group = [], max_candidates, b"", -1
    for i in range(max_candidates):
        if len(out) == count:
            break
        cand = cand_at(i % n)
        if i // 32 != group:
            group = i // 32
            digest = hashlib.sha256(seed + group.to_bytes(8, "little")).digest()
        if int(inc[cand]) * 255 >= max_inc * digest[i % 32]:
            out.append(cand)
            if len(out) == count:
                tried = i + 1
    found = len(out)
    return out + [NONE] * (count - found), found, tried


def sample_spec(seed: bytes, active, inc, max_inc: int, count: int, max_candidates: int):
    n = len(active)
    return _walk(lambda p: int(active[SH.compute_shuffled_index(p, n, seed)]), n, seed, inc, max_inc, count,
                 max_candidates)


def sample_rounds(seed: bytes, active, inc, max_inc: int, count: int, max_candidates: int):
    shuffled = SH.unshuffle_rounds(active, seed)
    return _walk(lambda p: int(shuffled[p]), len(active), seed, inc, max_inc, count, max_candidates)


def slot_seeds(epoch_seed: bytes, start_slot: int, slots: int = 32):
    """computeProposers' per-slot seeds (seed.ts:34): SHA256(epoch_seed || LE64(slot))"""
    return [hashlib.sha256(epoch_seed + (start_slot + i).to_bytes(8, "little")).digest() for i in range(slots)]


# ---- the cases of tests/test_gpu_sample.py, stated once (tests/test_sample_host.py checks on the
# CPU that each has the properties the GPU test relies on) ---------------------------------------
SIZES = [1, 2, 3, 255, 256, 257, 513, 65537]


def size_case(n: int):
    """(seed, active, increments, max_inc, count, max_candidates): acceptance 1/32"""
    seed = hashlib.sha256(b"gpu-sample" + n.to_bytes(4, "little")).digest()
    active = np.arange(n, dtype=np.uint32) * 3 + 11
    inc = np.ones(int(active[-1]) + 1, np.uint8)
    return seed, active, inc, 32, 512, 1 << 20


def passes_case():
    """acceptance 1/128 (increments 1 of max 255): `tried` lies past several passes"""
    seed = hashlib.sha256(b"gpu-sample-passes").digest()
    active = np.arange(700, dtype=np.uint32) + 1
    return seed, active, np.ones(701, np.uint8), 255, 512, 1 << 20


def proposers_case():
    """(epoch_seed, start_slot, active, increments): 32 slots, n = 1000, increments in 0..32"""
    rnd = np.random.default_rng(20261020)
    n = 1000
    active = np.arange(n, dtype=np.uint32) + 5
    inc = rnd.integers(0, 33, n + 5).astype(np.uint8)
    return hashlib.sha256(b"gpu-proposers").digest(), 6400, active, inc


def unfilled_case():
    """64 seeds, n = 3, every increment 0: a seed fills only where its random byte is 0"""
    seeds = [hashlib.sha256(b"z" + bytes([b])).digest() for b in range(64)]
    return seeds, np.array([4, 2, 7], np.uint32), np.zeros(8, np.uint8)


def range_case():
    """max_inc = 255, increments uniform in 0..255: the products need 16 bits"""
    rnd = np.random.default_rng(20261022)
    n = 300
    active = rnd.permutation(400)[:n].astype(np.uint32)
    inc = rnd.integers(0, 256, 400).astype(np.uint8)
    return hashlib.sha256(b"gpu-sample-range").digest(), active, inc, 255, 64, 1 << 16
