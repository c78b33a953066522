"""GPU check of k_line_pairs (lodestar_amd/csrc/k_steps.hip): the products of a lane's line pairs
taken out of k_step_acc into a kernel of their own, which stores them in place.

One call of requests of 1, 2, 3, 67, 68, 69, 127 and 128 sets and an empty one (465 sets), its
lines random canonical Fp2 values.  For the accumulator in registers and in LDS (MODE 0, 1) and 1,
2 and 4 lanes per set: the lanes' values G from k_step_acc on the raw lines equal those from
k_line_pairs + k_step_acc<.., true> bit for bit; single lines, the untouched third coefficient of a
pair's second line, and the slots past the sets' (the S_k pairs, the merged pair) are unchanged in
the buffer.  Outside the code under test: for one lane of the 3-set request and one of the 69-set
request, G is the pure-Python oracle's Fp12 product of the same lines with the same squarings.
The HIP side is tests/native/steps_selftest.hip (built by build(); test-only); the walk of a
lane's items is restated here as the loop step_lines ran (tests/test_steps_walk.py checks the
shared walk against the same restatement on the host)."""
import ctypes
import os

import numpy as np
import pytest

from oracle import bls12_381 as O
from tests import field_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libsteps_selftest.so")

pytestmark = pytest.mark.gpu

LINES = 68
SIZES = [3, 128, 1, 67, 0, 69, 2, 127, 68]  # request k's sets
P_TOP = O.P >> 352  # a top limb below p's keeps the value below p


def _levels():
    """level of each of the 68 lines: the doubling line of bit i = 62..0, then the addition line"""
    lvl = []
    for i in range(62, -1, -1):
        lvl.append(62 - i)
        if (O.X_ABS >> i) & 1:
            lvl.append(62 - i)
    assert len(lvl) == LINES
    return lvl


LVL = _levels()


def lane_items(n, t0, cnt):
    """step_lines' loop (k_steps.hip): (j, i, two lines at once) per iteration"""
    j, i = divmod(t0, n)
    out, c = [], 0
    while c < cnt:
        two = i + 1 < n and c + 1 < cnt
        out.append((j, i, two))
        i += 1 + two
        c += 1 + two
        if i >= n:
            i -= n
            j += 1
    return out


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("tests/native/libsteps_selftest.so missing: run __graft_entry__.build()")
    L = ctypes.CDLL(LIB)
    L.st_run.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32] + \
        [ctypes.c_void_p] * 5
    return L


@pytest.fixture(scope="module")
def call():
    """req_off, and the lines of every slot: (68, 72, n_pairs) words, each Fp coefficient below p"""
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint32)
    n_sets, n_req = int(off[-1]), len(SIZES)
    assert n_sets == 465
    n_pairs = n_sets + n_req + 1
    rng = np.random.default_rng(20240611)
    lines = rng.integers(0, 1 << 32, size=(LINES, 6, 12, n_pairs), dtype=np.uint64).astype(np.uint32)
    lines[:, :, 11, :] = rng.integers(0, P_TOP, size=(LINES, 6, n_pairs), dtype=np.uint64).astype(np.uint32)
    lines = np.ascontiguousarray(lines.reshape(LINES, 72, n_pairs))
    lines.setflags(write=False)
    return off, n_sets, n_req, n_pairs, lines


def run(lib, call, mode, split):
    off, n_sets, n_req, n_pairs, lines = call
    G_raw = np.zeros((144, n_sets * split), np.uint32)
    G_pre = np.full_like(G_raw, 0xFFFFFFFF)
    after = np.zeros_like(lines)
    rowoff = np.zeros(n_sets + 1, np.uint32)
    pos = np.zeros(n_req, np.uint32)
    rc = lib.st_run(n_req, off.ctypes.data, lines.ctypes.data, mode, split, G_raw.ctypes.data, G_pre.ctypes.data,
                    after.ctypes.data, rowoff.ctypes.data, pos.ctypes.data)
    assert rc == 0, "HIP call failed at steps_selftest.hip:%d" % rc
    return G_raw, G_pre, after, rowoff, pos


def fp_at(words, q):
    """the Fp values (out of Montgomery form) of a column of 12 k words"""
    col = words[:, q].reshape(-1, 12)
    return [C.unmont(v) for v in C.ints(col)]


def oracle_lane(lines, rowoff, r, n, t0, cnt):
    """Horner product of lines t0 .. t0 + cnt - 1 of the n-set request at position r"""
    acc, lvl = None, None
    for t in range(t0, t0 + cnt):
        j, i = divmod(t, n)
        c = fp_at(lines[j], int(rowoff[i]) + r)
        l0, l1, l4 = (c[0], c[1]), (c[2], c[3]), (c[4], c[5])
        line = ((l0, l1, O.F2_ZERO), (O.F2_ZERO, l4, O.F2_ZERO))
        if acc is not None and LVL[j] != lvl:  # one doubling step further: one squaring
            acc = O.f12_sqr(acc)
        lvl = LVL[j]
        acc = line if acc is None else O.f12_mul(acc, line)
    return acc


@pytest.mark.parametrize("split", [1, 2, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_line_pairs(lib, call, mode, split):
    off, n_sets, n_req, n_pairs, lines = call
    G_raw, G_pre, after, rowoff, pos = run(lib, call, mode, split)
    L = LINES // split
    # the row layout is what the walk below assumes: set i of request k at slot rowoff[i] + pos[k]
    assert sorted(pos.tolist()) == list(range(n_req)) and int(rowoff[max(SIZES)]) == n_sets
    assert [SIZES[k] for k in np.argsort(pos)] == sorted(SIZES, reverse=True)

    # 1. bit for bit
    assert G_raw.any() and np.array_equal(G_raw, G_pre)

    # 2. what k_line_pairs may write: the first line of a pair, words 0..47 of its second
    may = np.zeros(after.shape, bool)
    n_pair_items = 0
    for k, n in enumerate(SIZES):
        r = int(pos[k])
        for lane in range(n * split):
            t0 = LINES * (lane // split) + L * (lane % split)
            for j, i, two in lane_items(n, t0, L):
                if two:
                    may[j, :, int(rowoff[i]) + r] = True
                    may[j, :48, int(rowoff[i + 1]) + r] = True
                    n_pair_items += 1
    assert n_pair_items > 0 and not may[:, :, n_sets:].any()
    assert np.array_equal(after[~may], lines[~may])  # singles, the slots >= n_sets, a second line's l4
    assert (after[may] != lines[may]).mean() > 0.99  # (and the records were written)

    # 3. the oracle's product of the same lines, for one lane part of the 3- and of the 69-set request
    for n, lane in ((3, 1), (69, 1)):
        k = SIZES.index(n)
        r, h = int(pos[k]), split - 1
        t0 = LINES * lane + L * h
        want = [C.mont(c) for c in C.f12_flat(oracle_lane(lines, rowoff, r, n, t0, L))]
        q = int(rowoff[lane]) + r
        got = C.ints(G_pre[:, q * split + h].reshape(12, 12))
        assert got == want, (n, lane)
