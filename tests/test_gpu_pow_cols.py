"""GPU checks of the resident exponentiation a^((p-3)/4) (lodestar_amd/csrc/bls_fp_pow.h), one
primitive at a time and one element per lane: the entry and exit conversions, the resident
squaring and product on operands up to the documented bound 2p, the whole exponentiation, and
fp_pow_p34 itself, bit for bit against Python big integers.  The cases are those of the host
test (tests/pow_cols_cases.py); each operation is one launch of at most 512 elements.
The HIP side is tests/native/pow_selftest.hip (built by build(); test-only)."""
import ctypes
import os

import numpy as np
import pytest

from tests import pow_cols_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (LB_POW_SELFTEST: another build of the same self-test, e.g. with -DLB_POW_COLS=0)
LIB = os.environ.get("LB_POW_SELFTEST") or os.path.join(ROOT, "tests", "native", "libpow_selftest.so")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("tests/native/libpow_selftest.so missing: run __graft_entry__.build()")
    L = ctypes.CDLL(LIB)
    L.lbt_pow_op.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return L


def run(lib, op, a, b, wout):
    a = np.ascontiguousarray(np.array(a, np.uint32))
    out = np.zeros((a.shape[0], wout), np.uint32)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(np.array(b, np.uint32))
        bp = b.ctypes.data
    assert a.shape[0] <= 512
    rc = lib.lbt_pow_op(op, a.shape[0], a.ctypes.data, bp, out.ctypes.data)
    assert rc == 0, rc
    return out


def test_enter(lib):
    vals = C.CANONICAL + [C.R - 1, C.R - 2, 2 * C.P]  # the entry reads any 12-limb word
    out = run(lib, 0, [C.limbs(v) for v in vals], None, 13)
    assert [list(map(int, row)) for row in out] == [C.digits(v) for v in vals]


def test_leave(lib):
    out = run(lib, 1, [C.digits(v) for v in C.RESIDENT], None, 12)
    assert [C.from_limbs(row) for row in out] == [v % C.P for v in C.RESIDENT]


def test_resident_sqr(lib):
    out = run(lib, 2, [C.digits(v) for v in C.RESIDENT], None, 13)
    assert int(out.max()) <= C.M30
    assert [C.from_digits(row) for row in out] == [C.mont390(v * v) for v in C.RESIDENT]


def test_resident_mul(lib):
    out = run(lib, 3, [C.digits(v) for v in C.RESIDENT], [C.digits(v) for v in C.RESIDENT_B], 13)
    assert int(out.max()) <= C.M30
    assert [C.from_digits(row) for row in out] == [C.mont390(a * b) for a, b in zip(C.RESIDENT, C.RESIDENT_B)]


@pytest.mark.parametrize("op", [4, 5], ids=["resident", "fp_pow_p34"])
def test_pow_p34(lib, op):
    """The resident body, and fp_pow_p34 as this build's LB_POW_COLS wires it, on inputs < p."""
    out = run(lib, op, [C.limbs(v) for v in C.CANONICAL], None, 12)
    assert [C.from_limbs(row) for row in out] == [C.pow_expected(v) for v in C.CANONICAL]
