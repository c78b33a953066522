"""CPU precondition of tests/test_gpu_g1_edges.py: the torsion-shifted pubkey really is
the case only the G1 subgroup check can reject.  Without these three facts the GPU cases
could not fail."""
from oracle import bls12_381 as O
from tests import g1_edges_helper as H


def test_torsion_shifted_pubkey_precondition():
    pk, pk_s, _ = H.keys()
    # on E1, outside G1
    assert O.E1.on_curve(pk_s) and not O.g1_in_subgroup(pk_s) and O.g1_in_subgroup(pk)
    # the pairing cannot tell pk' from pk
    h = O.hash_to_g2(H.MSG)
    assert O.pairing(pk_s, h) == O.pairing(pk, h)
    # core verify rejects it; alone the set is False, beside a second valid set it is True
    shifted = H.sets()[0]
    assert not O.core_verify(pk_s, H.MSG, O.signature_from_bytes(shifted[2]))
    assert H.oracle_verdicts() == [False, True, False, True]
