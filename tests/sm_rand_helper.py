"""Python restatement of the randomized same-message aggregation (LB_SM_RANDOMIZED).

TEST INFRASTRUCTURE ONLY, on top of ``oracle.bls12_381`` and ``oracle.batch``.

For a call with seed ``seed``, set i is indexed over the whole call (0 <= i < n_sets) and
belongs to job j with message m_j:

* s_i = batch_scalar(seed, 0x80000000 | i): the call's DRBG in its GLV form, the index with its
  top bit set so these scalars never coincide with the merged check's r_k (indices < n_sets);
* a job of >= 2 sets: PK_j = sum s_i pk_i, S_j = sum s_i sig_i;
* a job of exactly one set is not multiplied: PK_j = pk_i, S_j = sig_i;
* an infinite decoded signature contributes the identity;
* a job that is empty, holds a signature failing Signature.fromBytes(validate=true) or a pubkey
  that fails to load, or whose aggregated key is infinite, is not fast: each set alone;
* otherwise (PK_j, m_j, S_j) is verified as one set; false -> each set alone.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

from oracle import batch as B
from oracle import bls12_381 as O

LB_SM_AGG_INDEX_FLAG = 0x80000000


def agg_scalar(seed: bytes, i: int) -> int:
    """s_i of set i of the call."""
    assert 0 <= i < LB_SM_AGG_INDEX_FLAG
    return B.batch_scalar(seed, LB_SM_AGG_INDEX_FLAG | i)


def _aggregate(pks: Sequence[bytes], sigs: Sequence[bytes], seed: bytes, base: int):
    """(PK, S) points of one job whose first set is set `base` of the call, or None (not aggregated)."""
    if len(pks) == 0:
        return None
    try:
        pk_pts = [O.g1_from_bytes(bytes(p)) for p in pks]
        sig_pts = [O.signature_from_bytes(bytes(s), validate=True) for s in sigs]
    except O.DeserializeError:
        return None
    if len(pks) == 1:
        agg_pk, agg_sig = pk_pts[0], sig_pts[0]
    else:
        agg_pk = agg_sig = None
        for k, (p, s) in enumerate(zip(pk_pts, sig_pts)):
            r = agg_scalar(seed, base + k)
            agg_pk = O.E1.add(agg_pk, O.g1_mul(p, r) if p is not None else None)
            agg_sig = O.E2.add(agg_sig, O.g2_mul(s, r) if s is not None else None)
    if agg_pk is None:
        return None
    return agg_pk, agg_sig


def randomized_aggregates(jobs, seed: bytes) -> Tuple[List[bytes], List[bytes], List[bool]]:
    """jobs: (pubkey encodings, signature bytes, message) per job, in call order.  Returns per
    job the aggregate's 96-byte key and 192-byte signature encodings and the bad flag; a bad
    job's encodings are all zero bytes (what lb_same_message_aggregates returns)."""
    pk_out, sig_out, bad = [], [], []
    base = 0
    for pks, sigs, _ in jobs:
        agg = _aggregate(pks, sigs, seed, base)
        base += len(pks)
        if agg is None:
            pk_out.append(bytes(96))
            sig_out.append(bytes(192))
            bad.append(True)
        else:
            pk_out.append(O.g1_to_bytes(agg[0], compressed=False))
            sig_out.append(O.g2_to_bytes(agg[1], compressed=False))
            bad.append(False)
    return pk_out, sig_out, bad


def verify_same_message_randomized(sets: Sequence[Tuple[bytes, bytes]], message: bytes, seed: bytes,
                                   index_base: int = 0) -> Tuple[List[bool], bool]:
    """oracle.batch.verify_same_message with the randomized sums: [(pubkey encoding, signature
    bytes)] of one job whose first set is set `index_base` of the call -> (per-set verdicts,
    fast_path_ok)."""
    if len(sets) == 0:
        return [], False
    agg = _aggregate([p for p, _ in sets], [s for _, s in sets], seed, index_base)
    if agg is not None:
        agg_bytes = O.g2_to_bytes(agg[1], compressed=False)
        if B.verify_signature_sets_maybe_batch([(agg[0], message, agg_bytes)]):
            return [True] * len(sets), True
    return [B.verify_signature_sets_maybe_batch([(pk, message, s)]) for pk, s in sets], False
