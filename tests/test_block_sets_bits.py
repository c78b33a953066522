"""BlockSignatureSetBuilder with committee_slices / sync_committee_list: attestations and the
sync aggregate as bits sets over device-resident index lists.  By the Python expansion they name
exactly the validators today's sets list; on the GPU both forms of a block verify alike."""
import os

import numpy as np
import pytest

import blocks_helper as BH
import shuffle_helper as SH
from lodestar_amd import block_sets as B
from lodestar_amd.verifier import SignatureSetType, pack_set_keys

GOLD = os.path.join(os.path.dirname(__file__), "golden")


class SliceBook:
    """Committees laid end to end in one index list, as an epoch's shuffling holds them:
    committee(slot, index) for today's form, slices(slot, index) for the bits form."""

    def __init__(self, committee):
        self._committee = committee
        self.where = {}
        self.entries = []

    def slices(self, slot, index, list_id=0):
        if (slot, index) not in self.where:
            members = list(self._committee(slot, index))
            self.where[(slot, index)] = (len(self.entries), len(members))
            self.entries += members
        start, n = self.where[(slot, index)]
        return list_id, start, n

    def array(self):
        return np.array(self.entries, np.uint32)


def set_indices(sets, lists):
    """Every set's validator indices: the descriptors' Python expansion for a package that
    packs, the keys themselves otherwise."""
    packed = pack_set_keys(sets)
    if packed is None:
        return None
    rows, pool, bits = packed
    off, idx = SH.expand_set_keys(rows, pool, bits.tobytes(), lists)
    return [idx[off[i]:off[i + 1]].tolist() for i in range(len(sets))]


def test_goerli_block_bits_sets_name_todays_indices():
    ssz = open(os.path.join(GOLD, "goerli_shadow_fork_block_13249.ssz"), "rb").read()
    blk = B.parse_signed_block(ssz, "bellatrix")
    sizes = {}
    for a in blk.attestations:
        n = (len(a.aggregation_bits) - 1) * 8 + a.aggregation_bits[-1].bit_length() - 1
        sizes[(int.from_bytes(a.data[0:8], "little"), int.from_bytes(a.data[8:16], "little"))] = n
    cfg = B.ChainConfig(bytes(32), [(0, bytes(4), "phase0"), (0, bytes([1, 0, 0, 0]), "altair"),
                                    (0, bytes([2, 0, 0, 0]), "bellatrix")])
    # committees of the fixture's sizes with contents of their own; a sync committee with duplicates
    comm = lambda s, i: [(1000 * i + 37 * s + 11 * k) % 50021 for k in range(sizes[(s, i)])]  # noqa: E731
    sync_members = [(13 * k) % 300 for k in range(512)]
    book = SliceBook(comm)
    today = B.BlockSignatureSetBuilder(BH.OracleRoots(), cfg, comm, lambda s: sync_members).build([ssz])[0]
    bits = B.BlockSignatureSetBuilder(BH.OracleRoots(), cfg, None, None, committee_slices=book.slices,
                                      sync_committee_list=1).build([ssz])[0]
    assert len(bits) == len(today) and len(blk.attestations) > 0
    assert [(s.signing_root, s.signature) for s in bits] == [(s.signing_root, s.signature) for s in today]
    n_bits = sum(1 for s in bits if s.type == SignatureSetType.bits)
    assert n_bits == len(blk.attestations) + 1  # every attestation and the sync aggregate
    got = set_indices(bits, {0: book.array(), 1: np.array(sync_members, np.uint32)})
    assert got is not None
    for s, t, ix in zip(bits, today, got):
        want = [t.pubkey.index] if t.pubkey is not None else [k.index for k in t.pubkeys]
        if s.type == SignatureSetType.bits:
            assert sorted(ix) == sorted(want) and len(ix) > 0  # (today's attestation sets are sorted)
        else:
            assert ix == want and s.type == t.type


def test_bitlist_of_another_length_is_refused():
    ssz = open(os.path.join(GOLD, "goerli_shadow_fork_block_13249.ssz"), "rb").read()
    cfg = B.ChainConfig(bytes(32), [(0, bytes(4), "phase0"), (0, bytes([1, 0, 0, 0]), "altair"),
                                    (0, bytes([2, 0, 0, 0]), "bellatrix")])
    with pytest.raises(B.SszError):
        B.BlockSignatureSetBuilder(BH.OracleRoots(), cfg, None, None, committee_slices=lambda s, i: (0, 0, 7),
                                   sync_committee_list=1).build([ssz])


@pytest.mark.gpu
def test_both_forms_verify_alike_on_the_gpu():
    """Two altair blocks with every operation kind under synthetic keys, the second with a wrong
    attestation signature: the same verdicts through index keys and through bits sets."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import workloads as W
    from lodestar_amd.verifier import DeviceBackend
    nv = 96
    b = DeviceBackend(0, seed_source=lambda: bytes(range(32)))
    try:
        keys = W.make_keys(b.dev, nv)
        assert b.dev.pubkey_table_append(keys.pks) == nv
        chain = BH.Chain(bytes(range(32)), [(0, bytes(4)), (2, bytes([1, 0, 0, 0]))])
        config = B.ChainConfig(bytes(range(32)), [(0, bytes(4), "phase0"), (2, bytes([1, 0, 0, 0]), "altair")])
        committee, sync = BH.committee_of(nv), BH.sync_committee_of(nv)
        blocks, parent = [], bytes(32)
        for n, slot in enumerate([70, 71]):
            def sign(sks, roots, corrupt=(n == 1)):
                sig = W.sign_many(b.dev, sks, roots)
                if corrupt and len(sig) > 8:
                    sig[1 + 2 + 2] = sig[0]  # the first attestation
                return sig
            ssz, _, root, _ = BH.make_block(sign, keys.sks, chain, slot, (7 * n) % nv, parent, committee, sync,
                                            n_atts=6, n_exits=2, n_prop_sl=1, n_att_sl=1, n_deposits=1,
                                            sync_participants=200, seed=n)
            blocks.append(ssz)
            parent = root
        today = B.BlockSignatureSetBuilder(b.dev, config, committee, sync).build(blocks)
        book = SliceBook(committee)
        bits = B.BlockSignatureSetBuilder(b.dev, config, None, None, committee_slices=book.slices,
                                          sync_committee_list=1).build(blocks)
        assert sum(1 for blk in bits for s in blk if s.type == SignatureSetType.bits) == 2 * (6 + 1)
        b.put_index_list(0, book.array())
        b.put_index_list(1, sync(70))
        v_today, e_today = b.verify_requests(today)
        v_bits, e_bits = b.verify_requests(bits)
        assert v_bits == v_today == [True, False] and e_bits == e_today == [0, 0]
        assert "expand_keys" in dict(b.dev.last_stage_times())
    finally:
        b.close()
