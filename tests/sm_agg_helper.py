"""Pure-Python restatement of the per-job aggregate signatures
(lb_verify_same_message_batch_agg, lb_aggregate_signature_groups) over oracle.bls12_381.

A job's aggregate is the plain sum of the decoded signatures of its sets that verified and
that the mask keeps -- Signature.aggregate(those).toBytes(): 96 compressed bytes, the
infinity encoding (0xc0, 95 zero bytes) for an empty sum.  Verdicts are inputs here (the
tests know them by construction), so no pairing is computed.
"""
from typing import List, Optional, Sequence, Tuple

from oracle import bls12_381 as O

INFINITY96 = bytes([0xC0]) + bytes(95)


def aggregate_bytes(signatures: Sequence[bytes], validate: bool = True) -> bytes:
    """Signature.aggregate([Signature.fromBytes(s, validate) ...]).toBytes()"""
    pts = [O.signature_from_bytes(s, validate=validate) for s in signatures]
    if not pts:  # (the oracle's aggregate refuses an empty list; the library writes infinity)
        return INFINITY96
    return O.g2_to_bytes(O.aggregate_g2(pts), compressed=True)


def expected_job_aggregates(jobs, verdicts: Sequence[Sequence[bool]],
                            mask: Optional[Sequence[Sequence[bool]]] = None,
                            validate: bool = True) -> List[Tuple[bytes, int]]:
    """jobs: (keys, signatures, root) per job; verdicts / mask: one flag per set per job
    (mask None: every set).  -> (sig96, count) per job.  validate=False skips the subgroup
    check of the summed signatures (a set with a true verdict has passed it on the device;
    the sum is the same, the Python ladder is 8x the decompression)."""
    out = []
    for j, (_, sigs, _) in enumerate(jobs):
        take = [s for i, s in enumerate(sigs) if verdicts[j][i] and (mask is None or mask[j][i])]
        out.append((aggregate_bytes(take, validate=validate), len(take)))
    return out


def expected_groups(groups: Sequence[Sequence[bytes]], no_check: bool = False) -> Tuple[List[bytes], List[int]]:
    """lb_aggregate_signature_groups: (sum per group, or 96 zero bytes; call-wide index of the
    group's first signature that fails to load, or -1)."""
    sums, bad, base = [], [], 0
    for g in groups:
        first = -1
        for i, s in enumerate(g):
            try:
                O.signature_from_bytes(s, validate=not no_check)
            except O.DeserializeError:
                first = base + i
                break
        bad.append(first)
        sums.append(bytes(96) if first >= 0 else aggregate_bytes(g, validate=not no_check))
        base += len(g)
    return sums, bad
