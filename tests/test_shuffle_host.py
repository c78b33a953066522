"""The two hashlib restatements of the swap-or-not shuffle (tests/shuffle_helper.py), the reference
of lb_index_list_shuffle's GPU tests: both reproduce the reference's unshuffleList vectors and
agree with each other around the 256-position digest boundary."""
import hashlib

import numpy as np
import pytest

import shuffle_helper as SH


def test_kat_both_forms():
    seed, cases = SH.load_kat()
    assert len(seed) == 32 and len(cases) == 2
    for inp, res in cases:
        assert SH.unshuffle_spec(inp, seed) == res
        assert SH.unshuffle_rounds(inp, seed).tolist() == res


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513, 5000])
def test_forms_agree(n):
    seed = hashlib.sha256(b"shuffle-host" + n.to_bytes(4, "little")).digest()
    active = (np.arange(n, dtype=np.uint32) * 7 + 3) % 100003  # not the identity
    got = SH.unshuffle_rounds(active, seed)
    assert got.tolist() == SH.unshuffle_spec(active.tolist(), seed)
    assert sorted(got.tolist()) == sorted(active.tolist())  # a permutation of the input
