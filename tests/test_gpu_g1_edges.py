"""G1 edges through the public C ABI: the torsion-shifted pubkey pk' = pk + T (on E1,
outside G1, invisible to the pairing; tests/g1_edges_helper.py and the CPU precondition in
tests/test_g1_torsion_precondition.py) on every path that takes a pubkey, and the G1
decoding edge encodings, mirroring the sig_decode list of tests/golden/make_golden.py.
A path that dropped or broke g1_in_subgroup would accept a pubkey the reference rejects.
Every expected value is the oracle's, computed at test time."""
import hashlib

import numpy as np
import pytest

from lodestar_amd.native import Device, pack_blobs
from oracle import batch as OB
from oracle import bls12_381 as O
from tests import g1_edges_helper as H
from tests.test_gpu_parity import interop_sk_be, run_requests

pytestmark = pytest.mark.gpu

ST_NOT_IN_GROUP = H.STATUS["POINT_NOT_IN_GROUP"]


def unc(pt):
    return O.g1_to_bytes(pt, compressed=False)


def as_request(sets):
    return [{"pks": [unc(p).hex() for p in pks], "msg": msg.hex(), "sig": sig.hex()} for pks, msg, sig in sets]


def test_verify_requests_torsion_shifted_pubkey(device_modes):
    """One call: [pk' set] (False), [pk' set, ordinary set] (True: the batch equation cannot
    see T), [aggregate set of pk' and pk2] (False), [ordinary set] (True)."""
    shifted, ordinary, agg = H.sets()
    reqs = [as_request(r) for r in ([shifted], [shifted, ordinary], [agg], [ordinary])]
    res = run_requests(device_modes, reqs)
    assert list(res.errors) == [0, 0, 0, 0]
    assert [bool(v) for v in res.valid] == H.oracle_verdicts()


def test_torsion_shifted_pubkey_in_a_large_call(device):
    """The 1-set pk' request inside a 1,025-set call (the steps + MSM pipeline): the merged
    check over all sets passes, so only the G1 check of the 1-set request can reject it.
    The other request holds 1,024 valid sets made by the device's signer (itself checked
    against the oracle in tests/test_gpu_parity.py)."""
    n = 1024
    sks = [interop_sk_be(i) for i in range(n)]
    msgs = [hashlib.sha256(b"g1-edges" + i.to_bytes(4, "little")).digest() for i in range(n)]
    pks = device.sk_to_pk(sks)
    sigs = device.sign(sks, msgs)
    (pk_s,), msg_s, sig_s = H.sets()[0]
    blob, offs = pack_blobs([sig_s] + sigs)
    res = device.verify_requests(np.array([0, 1, n + 1], np.uint32), np.frombuffer(unc(pk_s) + b"".join(pks), np.uint8),
                                 None, np.frombuffer(msg_s + b"".join(msgs), np.uint8), blob, offs, bytes(32))
    assert list(res.errors) == [0, 0]
    assert [bool(v) for v in res.valid] == [H.oracle_verdicts()[0], True]


def test_same_message_job_with_torsion_shifted_pubkey(device):
    """Per-set verdicts of a same-message job holding pk' == oracle.batch.verify_same_message."""
    _, pk_s, pk2 = H.keys()
    sig0 = H.sets()[0][2]
    sig1 = O.g2_to_bytes(O.sign(O.interop_secret_key(1), H.MSG))
    want = OB.verify_same_message([(pk_s, sig0), (pk2, sig1)], H.MSG)
    assert want == ([False, True], False)
    got = device.verify_same_message([unc(pk_s), unc(pk2)], [sig0, sig1], H.MSG, bytes(32))
    assert got == want


def test_pubkeys_from_bytes_rejects_torsion_shifted_pubkey(device):
    _, pk_s, pk2 = H.keys()
    for compressed in (True, False):
        keys = [O.g1_to_bytes(p, compressed=compressed) for p in (pk_s, pk2, pk_s)]
        out, st = device.pubkeys_from_bytes(keys)
        assert [H.pubkey_expect(k) for k in keys] == [(ST_NOT_IN_GROUP, H.INF96), (0, unc(pk2)), (ST_NOT_IN_GROUP, H.INF96)]
        assert st == [ST_NOT_IN_GROUP, 0, ST_NOT_IN_GROUP]
        assert out == [H.INF96, unc(pk2), H.INF96]


def test_pubkey_table_takes_torsion_shifted_pubkey_and_requests_reject_it():
    """lb_pubkey_table_append does not validate (its contract); a by-index 1-set request on
    that entry is False, the same request on an ordinary entry True."""
    shifted, ordinary, _ = H.sets()
    dev = Device(0)
    try:
        assert dev.pubkey_table_append([unc(shifted[0][0]), unc(ordinary[0][0])]) == 2
        assert dev.pubkey_table_read(0, 1) == [unc(shifted[0][0])]
        blob, offs = pack_blobs([shifted[2], ordinary[2]])
        res = dev.verify_requests(np.array([0, 1, 2], np.uint32), None, np.array([0, 1, 2], np.uint32),
                                  np.frombuffer(shifted[1] + ordinary[1], np.uint8), blob, offs, bytes(32),
                                  pk_indices=np.array([0, 1], np.uint32))
        assert list(res.errors) == [0, 0]
        assert [bool(v) for v in res.valid] == [H.oracle_verdicts()[0], H.oracle_verdicts()[3]]
    finally:
        dev.close()


def g1_decode_cases():
    """(name, bytes) per encoding length, mirroring the G2 sig_decode list."""
    P = O.P
    pk, pk_s, _ = H.keys()
    gc, gu = O.g1_to_bytes(pk), unc(pk)
    other = bytearray(gc)
    other[0] ^= 0x20
    x_bad = next(x for x in range(5, 100) if O.fp_sqrt(x ** 3 + 4) is None)
    raw = (4, O.fp_sqrt(68))

    def cx(x, flags=0x80):
        b = bytearray(x.to_bytes(48, "big"))
        b[0] |= flags
        return bytes(b)

    c48 = [("valid compressed", gc), ("valid compressed, other sign", bytes(other)),
           ("infinity compressed", bytes([0xC0]) + bytes(47)),
           ("infinity with junk", bytes([0xC0]) + bytes(46) + b"\x01"),
           ("infinity flag with sign bit", bytes([0xE0]) + bytes(47)),
           ("uncompressed bit with compressed length", bytes([gc[0] & 0x1F]) + gc[1:]),
           ("x = p", cx(P)), ("x = p + 1", cx(P + 1)), ("x = p - 1", cx(P - 1)), ("x = p, sign bit", cx(P, 0xA0)),
           ("no curve point at x", cx(x_bad)), ("x = 0", cx(0)), ("x = 0, sign bit", cx(0, 0xA0)),
           ("not in subgroup", O.g1_to_bytes(raw)), ("torsion-shifted", O.g1_to_bytes(pk_s)),
           ("generator", O.g1_to_bytes(O.G1)), ("48 zero bytes", bytes(48))]
    yp = bytearray(gu)
    yp[95] ^= 1
    c96 = [("valid uncompressed", gu), ("infinity uncompressed", H.INF96),
           ("infinity with junk", bytes([0x40]) + bytes(94) + b"\x01"),
           ("infinity flag with sign bit", bytes([0x60]) + bytes(95)),
           ("compressed bit with uncompressed length", bytes([0x80]) + bytes(95)),
           ("compressed point padded to 96", gc + bytes(48)),
           ("x = p", P.to_bytes(48, "big") + gu[48:]), ("x = p + 1", (P + 1).to_bytes(48, "big") + gu[48:]),
           ("y perturbed", bytes(yp)), ("(0, 0)", bytes(96)), ("y = p", gu[:48] + P.to_bytes(48, "big")),
           ("(0, 2)", bytes(48) + (2).to_bytes(48, "big")), ("(0, p - 2)", bytes(48) + (P - 2).to_bytes(48, "big")),
           ("sign flag on an uncompressed key", bytes([gu[0] | 0x20]) + gu[1:]),
           ("infinity flag on an uncompressed key", bytes([gu[0] | 0x40]) + gu[1:]),
           ("not in subgroup", unc(raw)), ("torsion-shifted", unc(pk_s))]
    return c48, c96


def test_g1_decode_edges(device):
    """lb_pubkeys_from_bytes == O.g1_from_bytes followed by the infinity and subgroup rules of
    k_pubkey_validate: status and 96-byte output, for each encoding length."""
    for cases in g1_decode_cases():
        names = [c[0] for c in cases]
        assert len(set(names)) == len(names)
        out, st = device.pubkeys_from_bytes([c[1] for c in cases])
        want = [H.pubkey_expect(c[1]) for c in cases]
        assert sorted({w[0] for w in want}) == [0, 1, 2, 3, 4]  # every status occurs
        for (name, _), s, o, (ws, wo) in zip(cases, st, out, want):
            assert (s, o) == (ws, wo), name
