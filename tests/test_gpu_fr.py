"""GPU checks of the one-lane scalar field (lodestar_amd/csrc/bls_fr.h) against Python
integers: add, sub, neg, Montgomery mul and sqr, pow, inversion and the byte codecs, at
the operands where a carry chain, the conditional subtraction or the canonical test can
go wrong.  Elements go in and come out as raw Montgomery limbs (R = 2^256) and are
converted here.  The HIP side is tests/native/fr_selftest.hip (built by build(); test-only)."""
import ctypes
import os
import random

import numpy as np
import pytest

from tests.kzg_helper import R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("LB_FR_SELFTEST") or os.path.join(ROOT, "tests", "native", "libfr_selftest.so")
MONT = 1 << 256
MONT_INV = pow(MONT, -1, R)

pytestmark = pytest.mark.gpu

F_ADD, F_SUB, F_NEG, F_MUL, F_SQR, F_INV, F_POW = range(7)
F_MUL_ALIAS, F_ADD_ALIAS, F_SUB_ALIAS = 10, 11, 12
F_FROM_BE, F_TO_BE, F_REDUCE = 20, 21, 22

rng = random.Random(20240)
# 0, 1, r-1, r-2, 2^255 - 1 reduced, values around the limb boundaries, and random ones
EDGE = [0, 1, 2, R - 1, R - 2, (2 ** 255 - 1) % R, 2 ** 32 - 1, 2 ** 32, 2 ** 224, 2 ** 254, (R - 1) // 2,
        (R + 1) // 2, MONT % R, MONT_INV, R - MONT % R] + [rng.randrange(R) for _ in range(9)]
# pairs whose sum is r and r +- 1 (the conditional subtraction's boundary)
SUM_PAIRS = [(a, (R - a + d) % R) for a in (1, 5, (R - 1) // 2, R - 1, rng.randrange(1, R)) for d in (-1, 0, 1)]
PAIRS = [(a, b) for a in EDGE for b in EDGE] + SUM_PAIRS


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("tests/native/libfr_selftest.so missing: run __graft_entry__.build()")
    L = ctypes.CDLL(LIB)
    L.lbt_fr_op.argtypes = [ctypes.c_int, ctypes.c_uint32] + [ctypes.c_void_p] * 4
    return L


def limbs(v):
    return [(v >> (32 * j)) & 0xFFFFFFFF for j in range(8)]


def mont(v):
    return limbs(v % R * MONT % R)


def unmont(row):
    v = sum(int(x) << (32 * j) for j, x in enumerate(row))
    assert v < R, "result not fully reduced"
    return v * MONT_INV % R


def run(lib, op, a_rows, b_rows=None):
    n = len(a_rows)
    a = np.array(a_rows, dtype=np.uint32).reshape(n, 8)
    b = np.array(b_rows if b_rows is not None else [[0] * 8] * n, dtype=np.uint32).reshape(n, 8)
    out = np.zeros((n, 8), np.uint32)
    flag = np.zeros(n, np.uint32)
    rc = lib.lbt_fr_op(op, n, a.ctypes.data, b.ctypes.data, out.ctypes.data, flag.ctypes.data)
    assert rc == 0, f"hip error {rc}"
    return out, flag


@pytest.mark.parametrize("op,alias,fn", [
    (F_ADD, F_ADD_ALIAS, lambda a, b: (a + b) % R),
    (F_SUB, F_SUB_ALIAS, lambda a, b: (a - b) % R),
    (F_MUL, None, lambda a, b: a * b % R),
])
def test_binary_ops(lib, op, alias, fn):
    want = [fn(a, b) for a, b in PAIRS]
    for o in (op, alias):
        if o is None:
            continue
        out, _ = run(lib, o, [mont(a) for a, _ in PAIRS], [mont(b) for _, b in PAIRS])
        assert [unmont(r) for r in out] == want, o


def test_unary_ops(lib):
    rows = [mont(a) for a in EDGE]
    for op, fn in ((F_NEG, lambda a: (-a) % R), (F_SQR, lambda a: a * a % R), (F_MUL_ALIAS, lambda a: a * a % R),
                   (F_INV, lambda a: pow(a, R - 2, R))):
        out, _ = run(lib, op, rows)
        assert [unmont(r) for r in out] == [fn(a) for a in EDGE], op


def test_pow(lib):
    exps = [0, 1, 2, R - 2, R - 1, 2 ** 256 - 1, 4096, rng.getrandbits(256)]
    cases = [(a, e) for a in (0, 1, 7, R - 1, rng.randrange(R)) for e in exps]
    out, _ = run(lib, F_POW, [mont(a) for a, _ in cases], [limbs(e) for _, e in cases])
    assert [unmont(r) for r in out] == [pow(a, e, R) for a, e in cases]


def be_words(b32):
    """32 bytes as the 8 words a byte-addressed buffer holds on a little-endian host."""
    return list(np.frombuffer(b32, dtype="<u4"))


def test_read_bytes_accepts_canonical_and_rejects_r_and_above(lib):
    good = EDGE + [R - 1]
    bad = [R, R + 1, 2 ** 256 - 1, 2 ** 255, R + 2 ** 32]
    vals = good + bad
    out, flag = run(lib, F_FROM_BE, [be_words(v.to_bytes(32, "big")) for v in vals])
    assert list(flag) == [1] * len(good) + [0] * len(bad)
    assert [unmont(r) for r in out[:len(good)]] == good
    assert [unmont(r) for r in out[len(good):]] == [0] * len(bad)


def test_write_bytes_is_canonical_big_endian(lib):
    out, _ = run(lib, F_TO_BE, [mont(a) for a in EDGE])
    assert [out[i].tobytes() for i in range(len(EDGE))] == [a.to_bytes(32, "big") for a in EDGE]


def test_reduce_any_256_bit_value(lib):
    """hash_to_bls_field's reduction: up to two subtractions, full-length carries included."""
    vals = [0, 1, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 2 ** 255 - 1, 2 ** 255, 2 ** 256 - 1,
            2 ** 256 - 2 ** 32] + [rng.getrandbits(256) for _ in range(8)]
    rows = [[(v >> (32 * (7 - k))) & 0xFFFFFFFF for k in range(8)] for v in vals]
    out, _ = run(lib, F_REDUCE, rows)
    assert [unmont(r) for r in out] == [v % R for v in vals]
