"""The resident exponentiation a^((p-3)/4) on 30-bit columns (lodestar_amd/csrc/bls_fp_pow.h)
against Python big integers, on the host (g++ build of the same header): the entry and exit
conversions, the resident squaring and product on operands up to the documented bound 2p, and
the whole exponentiation, bit for bit; and the exponent the window program encodes.  Cases:
tests/pow_cols_cases.py.  A stand-alone build of the same file runs under
-fsanitize=undefined where the host compiler has it (the shifts are the risk)."""
import ctypes
import os
import subprocess

import pytest

from tests import pow_cols_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "pow_cols_host.cpp")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("powcols") / "libpow_cols_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC])
    return ctypes.CDLL(out)


def _u32(vals):
    return (ctypes.c_uint32 * len(vals))(*vals)


def test_window_program_exponent(lib):
    win = [lib.pw_win(k) for k in range(lib.pw_win_steps())]
    assert C.window_exponent(win) == (C.P - 3) // 4


def test_enter_leave(lib):
    d = (ctypes.c_uint32 * 13)()
    r = (ctypes.c_uint32 * 12)()
    for v in C.CANONICAL:
        lib.pw_enter(d, _u32(C.limbs(v)))
        assert list(d) == C.digits(v), v
        lib.pw_leave(r, d)
        assert C.from_limbs(r) == v, v
    # the exit makes any value below 2p canonical
    for v in C.RESIDENT:
        lib.pw_leave(r, _u32(C.digits(v)))
        assert C.from_limbs(r) == v % C.P, v
    # the entry reads any 12-limb word
    for v in (C.R - 1, C.R - 2, 2 * C.P):
        lib.pw_enter(d, _u32(C.limbs(v)))
        assert list(d) == C.digits(v), v


def test_resident_sqr_mul(lib):
    r = (ctypes.c_uint32 * 13)()
    for a, b in zip(C.RESIDENT, C.RESIDENT_B):
        lib.pw_sqr(r, _u32(C.digits(a)))
        v = C.from_digits(r)
        assert v == C.mont390(a * a) and v < 2 * C.P and max(r) <= C.M30, a
        lib.pw_mul(r, _u32(C.digits(a)), _u32(C.digits(b)))
        v = C.from_digits(r)
        assert v == C.mont390(a * b) and v < 2 * C.P and max(r) <= C.M30, (a, b)


def test_pow_p34(lib):
    r = (ctypes.c_uint32 * 12)()
    for v in C.CANONICAL:
        lib.pw_pow_p34(r, _u32(C.limbs(v)))
        assert C.from_limbs(r) == C.pow_expected(v), v


def test_standalone_under_ubsan(tmp_path):
    exe = str(tmp_path / "pow_cols_main")
    base = ["g++", "-O1", "-std=c++17", "-DPOW_COLS_MAIN", "-o", exe, SRC]
    san = subprocess.run(base + ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"], capture_output=True)
    if san.returncode != 0:  # no sanitizer runtime with this compiler: the plain program still cross-checks
        subprocess.check_call(base)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.stdout, res.stderr)
