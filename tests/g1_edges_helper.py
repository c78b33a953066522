"""The torsion-shifted pubkey fixture shared by tests/test_g1_torsion_precondition.py
(CPU) and tests/test_gpu_g1_edges.py (GPU).

pk' = pk + T with pk the interop key 0 and T = [r] * (4, sqrt(4^3 + 4)) a point of the
cofactor torsion of E1: pk' is on the curve and outside G1, yet e(pk', H(m)) = e(pk, H(m)),
so the pairing equation accepts pk's signature under pk' and only the G1 subgroup check
rejects it.  Every expected verdict is the oracle's, computed once per session."""
import functools
import hashlib

from oracle import batch as OB
from oracle import bls12_381 as O

STATUS = {"BAD_ENCODING": 1, "POINT_NOT_ON_CURVE": 2, "POINT_NOT_IN_GROUP": 3, "PK_INFINITY": 4}
INF96 = bytes([0x40]) + bytes(95)
MSG = hashlib.sha256(b"torsion-shifted pubkey").digest()
MSG2 = hashlib.sha256(b"an ordinary set").digest()


@functools.lru_cache(None)
def torsion_point():
    y = O.fp_sqrt(4 ** 3 + 4)
    assert y is not None
    T = O.g1_mul((4, y), O.R)
    assert T is not None and O.E1.on_curve(T)
    return T


@functools.lru_cache(None)
def keys():
    """(pk, pk', pk2) as oracle points."""
    pk = O.sk_to_pk(O.interop_secret_key(0))
    return pk, O.g1_add(pk, torsion_point()), O.sk_to_pk(O.interop_secret_key(1))


@functools.lru_cache(None)
def sets():
    """(shifted, ordinary, aggregate): (pubkey points, message, signature bytes) with
    shifted = pk' under pk's signature, ordinary = a valid set of key 1, aggregate = keys
    (pk', pk2) under the sum of both signatures on MSG."""
    sk0, sk1 = O.interop_secret_key(0), O.interop_secret_key(1)
    _, pk_s, pk2 = keys()
    sig0 = O.sign(sk0, MSG)
    shifted = ([pk_s], MSG, O.g2_to_bytes(sig0))
    ordinary = ([pk2], MSG2, O.g2_to_bytes(O.sign(sk1, MSG2)))
    agg = ([pk_s, pk2], MSG, O.g2_to_bytes(O.E2.add(sig0, O.sign(sk1, MSG))))
    return shifted, ordinary, agg


def _oracle_set(s):
    pks, msg, sig = s
    return (O.aggregate_g1(list(pks)), msg, sig)


@functools.lru_cache(None)
def oracle_verdicts():
    """The oracle's verdicts for the four requests of the GPU test: [shifted],
    [shifted, ordinary], [aggregate], [ordinary]."""
    shifted, ordinary, agg = sets()
    reqs = [[shifted], [shifted, ordinary], [agg], [ordinary]]
    return [OB.verify_signature_sets_maybe_batch([_oracle_set(s) for s in r]) for r in reqs]


def pubkey_expect(b):
    """(status, 96-byte output) of PublicKey.fromBytes(b, affine, validate = true): O.g1_from_bytes,
    then the infinity and subgroup rules of k_pubkey_validate; a rejected key leaves the
    infinity encoding."""
    try:
        pt = O.g1_from_bytes(b)
    except O.DeserializeError as e:
        return STATUS[str(e).split(":")[0]], INF96
    if pt is None:
        return STATUS["PK_INFINITY"], INF96
    if not O.g1_in_subgroup(pt):
        return STATUS["POINT_NOT_IN_GROUP"], INF96
    return 0, O.g1_to_bytes(pt, compressed=False)
