"""GPU checks of the field primitives added for lazy reduction (fp_mulw, fp_redc,
the lazy Fp2 product) and of the register-window exponentiation, on edge cases
no hashed input reaches: 0, 1, p - 1, all-ones limbs, and inputs up to 2p where
the documented bound allows them, and (second half of this file) of the rest of the
one-lane tower Fp ... Fp12.  Expected values are Python big integers.
The HIP side is tests/native/field_selftest.hip (built by build(); test-only)."""
import ctypes
import os
import random

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (LB_FIELD_SELFTEST: another build of the same self-test)
LIB = os.environ.get("LB_FIELD_SELFTEST") or os.path.join(ROOT, "tests", "native", "libfield_selftest.so")
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 1 << 384
RINV = pow(R, -1, P)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("tests/native/libfield_selftest.so missing: run __graft_entry__.build()")
    L = ctypes.CDLL(LIB)
    L.lbt_field_op.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return L


def limbs(vals, n):
    out = np.zeros((len(vals), n), np.uint32)
    for i, v in enumerate(vals):
        for j in range(n):
            out[i, j] = (v >> (32 * j)) & 0xFFFFFFFF
    return out


def ints(arr):
    return [sum(int(x) << (32 * j) for j, x in enumerate(row)) for row in arr]


def run(lib, op, a, b, wout):
    n = a.shape[0]
    out = np.zeros((n, wout), np.uint32)
    a = np.ascontiguousarray(a)
    bp = None
    if b is not None:
        b = np.ascontiguousarray(b)
        bp = b.ctypes.data
    rc = lib.lbt_field_op(op, n, a.ctypes.data, bp, out.ctypes.data)
    assert rc == 0, rc
    return out


EDGE = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (1 << 381) - 1, (1 << 352) - 1, 0xFFFFFFFF, 1 << 380]


def edge_and_random(k, bound, seed):
    rng = random.Random(seed)
    vals = [v % bound for v in EDGE] + [rng.randrange(bound) for _ in range(k)]
    return vals


def test_fp2_mul_lazy(lib):
    """Karatsuba with lazy reduction: inputs < p (the tower keeps them there) and up
    to 2p (the bound the reduction argument allows), output canonical."""
    rng = random.Random(5)
    cases = []
    for bound in (P, 2 * P):
        vals = edge_and_random(60, bound, 9 + bound % 7)
        for _ in range(300):
            cases.append(tuple(rng.choice(vals) for _ in range(4)))
    a = np.concatenate([limbs([c[0] for c in cases], 12), limbs([c[1] for c in cases], 12)], axis=1)
    b = np.concatenate([limbs([c[2] for c in cases], 12), limbs([c[3] for c in cases], 12)], axis=1)
    out = run(lib, 0, a, b, 24)
    r0, r1 = ints(out[:, :12]), ints(out[:, 12:])
    for (a0, a1, b0, b1), c0, c1 in zip(cases, r0, r1):
        assert c0 == (a0 * b0 - a1 * b1) * RINV % P, (a0, a1, b0, b1)
        assert c1 == (a0 * b1 + a1 * b0) * RINV % P, (a0, a1, b0, b1)


def test_mulw_redc(lib):
    xs = edge_and_random(200, R, 1)
    ys = list(reversed(edge_and_random(200, R, 2)))
    w = run(lib, 1, limbs(xs, 12), limbs(ys, 12), 24)
    assert ints(w) == [x * y for x, y in zip(xs, ys)]
    rng = random.Random(3)
    ws = [0, 1, P * R - 1, P * P, 2 * P * P - 1, R - 1, R * R // 16] + [rng.randrange(P * R) for _ in range(300)]
    r = run(lib, 2, limbs(ws, 24), None, 12)
    assert ints(r) == [v * RINV % P for v in ws]


def test_pow_p34(lib):
    """a^((p-3)/4) on Montgomery representatives (register-window exponentiation)."""
    xs = edge_and_random(200, P, 4)
    r = run(lib, 3, limbs([x * R % P for x in xs], 12), None, 12)
    e = (P - 3) // 4
    assert ints(r) == [pow(x, e, P) * R % P for x in xs]


def test_fp_mul(lib):
    xs = edge_and_random(200, P, 6)
    ys = edge_and_random(200, P, 7)
    r = run(lib, 4, limbs(xs, 12), limbs(ys, 12), 12)
    assert ints(r) == [x * y * RINV % P for x, y in zip(xs, ys)]


def test_fp_sqr(lib):
    xs = edge_and_random(200, P, 8)
    r = run(lib, 5, limbs(xs, 12), None, 12)
    assert ints(r) == [x * x * RINV % P for x in xs]


# ---------------------------------------------------------------------------------------
# The rest of the tower through the second entry point (lbt_field_op2): modular add/sub
# asm in every aliasing form the product uses, inversion, square roots, sign rules, byte
# conversions, Fp2 ... Fp12 including the sparse products, Frobenius and the cyclotomic
# squaring.  Cases and Python-integer expectations: tests/field_cases.py.
# ---------------------------------------------------------------------------------------
from oracle import bls12_381 as O  # noqa: E402
from tests import field_cases as C  # noqa: E402

(F_ADD, F_SUB, F_NEG, F_DBL, F_MUL3, F_ADD2_PLAIN, F_INV, F_SQRT, F_IS_SQUARE, F_LEX, F_PARITY, F_TO_MONT, F_FROM_MONT,
 F_FROM_BE48, F_TO_BE48, F_MUL, F_SQR) = range(100, 117)
(F2_ADD, F2_SUB, F2_SUBADD, F2_DBL, F2_NEG, F2_CONJ, F2_MUL_XI, F2_SQR, F2_MUL_FP, F2_MUL3, F2_INV, F2_SGN0, F2_LEX,
 F2_SQRT, FW_KCOMBINE, F2_MUL) = range(200, 216)
F6_MUL, F6_MUL_01, F6_MUL_1, F6_MUL_12, F6_MUL_V, F6_INV = range(300, 306)
F12_MUL, F12_SQR, F12_CONJ, F12_INV = range(400, 404)
F12_MUL_LINE, F12_LINE_LINE, F12_FROB1, F12_FROB2, F12_FROB3, F12_CYC_SQR, F12_IS_ONE = range(450, 457)

# aliasing forms (field_selftest.hip): distinct, r is a, r is b, a is b, r is a is b
BIN_VARS = [0, 1, 2, 3, 4]
UN_VARS = [0, 1]


@pytest.fixture(scope="module")
def lib2(lib):
    lib.lbt_field_op2.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p]
    lib.lbt_field_op2_widths.argtypes = [ctypes.c_int, ctypes.c_void_p]
    return lib


def run2(lib, op, var, a, b=None):
    """a, b: lists of rows of Fp coefficients (raw integers < 2^384) or uint32 arrays."""
    w = (ctypes.c_uint32 * 3)()
    assert lib.lbt_field_op2_widths(op, w) == 0, op
    wa, wb, wo = w

    def arr(x, width):
        if not isinstance(x, np.ndarray):
            x = C.limbs([v for row in x for v in row], 12)
        x = np.ascontiguousarray(x, np.uint32).reshape(-1, width)
        return x

    a = arr(a, wa)
    n = a.shape[0]
    bp = None
    if wb:
        b = arr(b, wb)
        assert b.shape[0] == n
        bp = b.ctypes.data
    out = np.zeros((n, wo), np.uint32)
    rc = lib.lbt_field_op2(op, var, n, a.ctypes.data, bp, out.ctypes.data)
    assert rc == 0, rc
    return out


def rows(out, k):
    """uint32 (n, 12 k [+ flag]) -> n rows of k integers."""
    return [C.ints(r[:12 * k].reshape(k, 12)) for r in out]


def m12(vals):
    return [[C.mont(c) for c in C.f12_flat(v)] for v in vals]


def m6(vals):
    return [[C.mont(c) for c in C.f6_flat(v)] for v in vals]


def m2(vals):
    return [[C.mont(v[0]), C.mont(v[1])] for v in vals]


def un12(out):
    return [C.f12_unflat([C.unmont(c) for c in r]) for r in rows(out, 12)]


def un6(out):
    return [C.f6_unflat([C.unmont(c) for c in r]) for r in rows(out, 6)]


def un2(out):
    return [tuple(C.unmont(c) for c in r) for r in rows(out, 2)]


def alias(var, xs, ys):
    """The operands the routine really sees: forms 3 and 4 pass a as b."""
    return (xs, xs) if var >= 3 else (xs, ys)


# ---- Fp ---------------------------------------------------------------------------------
@pytest.mark.parametrize("var", BIN_VARS)
def test_fp_add_sub(lib2, var):
    pairs = C.addsub_pairs()
    xs, ys = [[a] for a, _ in pairs], [[b] for _, b in pairs]
    ea, eb = alias(var, xs, ys)
    got = rows(run2(lib2, F_ADD, var, xs, ys), 1)
    assert got == [[(a[0] + b[0]) % P] for a, b in zip(ea, eb)]
    got = rows(run2(lib2, F_SUB, var, xs, ys), 1)
    assert got == [[(a[0] - b[0]) % P] for a, b in zip(ea, eb)]


def test_fp_add_equal_values_distinct_objects(lib2):
    """a and b hold the same value in two objects (form 0), beside fp_add(r, a, a) above."""
    xs = [[v] for v in C.EDGE + [a for a, _ in C.addsub_pairs()[:200]]]
    xs = [[x[0] % P] for x in xs]
    assert rows(run2(lib2, F_ADD, 0, xs, xs), 1) == [[2 * x[0] % P] for x in xs]
    assert rows(run2(lib2, F_SUB, 0, xs, xs), 1) == [[0] for _ in xs]


@pytest.mark.parametrize("var", UN_VARS)
def test_fp_neg_dbl_mul3(lib2, var):
    xs = [[v] for v in edge_and_random(200, P, 11) + [(P + 1) // 2, (P + 2) // 3, (2 * P + 2) // 3, P // 3, 1 << 352]]
    assert rows(run2(lib2, F_NEG, var, xs), 1) == [[(-x[0]) % P] for x in xs]
    assert rows(run2(lib2, F_DBL, var, xs), 1) == [[2 * x[0] % P] for x in xs]
    assert rows(run2(lib2, F_MUL3, var, xs), 1) == [[3 * x[0] % P] for x in xs]


@pytest.mark.parametrize("var", BIN_VARS)
def test_fp_mul_sqr_aliased(lib2, var):
    xs = [[v] for v in edge_and_random(100, P, 12)]
    ys = [[v] for v in reversed(edge_and_random(100, P, 13))]
    ea, eb = alias(var, xs, ys)
    assert rows(run2(lib2, F_MUL, var, xs, ys), 1) == [[a[0] * b[0] * RINV % P] for a, b in zip(ea, eb)]
    if var in UN_VARS:
        assert rows(run2(lib2, F_SQR, var, xs), 1) == [[x[0] * x[0] * RINV % P] for x in xs]


@pytest.mark.parametrize("var", [0, 3])
def test_fp_add2_plain(lib2, var):
    """(a0 + a1, b0 + b1) without reduction (the Karatsuba operands of fp2_mul)."""
    pairs = C.addsub_pairs()
    a = [[p[0], p[1]] for p in pairs]
    b = [[p[1], p[0]] for p in reversed(pairs)]
    got = rows(run2(lib2, F_ADD2_PLAIN, var, a, b), 2)
    if var == 3:
        assert got == [[2 * x[0], 2 * y[0]] for x, y in zip(a, b)]
    else:
        assert got == [[x[0] + x[1], y[0] + y[1]] for x, y in zip(a, b)]


@pytest.mark.parametrize("var", UN_VARS)
def test_fp_inv(lib2, var):
    """The gfx950 lowering of bls_inv.h: Montgomery in, Montgomery out, inv(0) = 0."""
    xs = C.inv_inputs()
    got = rows(run2(lib2, F_INV, var, [[x] for x in xs]), 1)
    for x, (r,) in zip(xs, got):
        assert r == (pow(x, -1, P) * R * R % P if x else 0), hex(x)


@pytest.mark.parametrize("var", UN_VARS)
def test_fp_sqrt_is_square(lib2, var):
    rng = random.Random(21)
    xs = [0, 1, P - 1, 4, 2, 3, P - 4, (P - 1) // 2, (P + 1) // 2] + [rng.randrange(P) for _ in range(200)]
    xs += [x * x % P for x in xs[:40]]
    a = [[C.mont(x)] for x in xs]
    out = run2(lib2, F_SQRT, var, a)
    sq = run2(lib2, F_IS_SQUARE, 0, a)
    n_sq = 0
    for x, (r,), row, s in zip(xs, rows(out, 1), out, sq):
        want = O.fp_is_square(x)
        assert bool(row[12]) == want, hex(x)
        assert bool(s[0]) == want, hex(x)
        if want:
            n_sq += 1
            assert r < P and C.unmont(r) ** 2 % P == x, hex(x)
    assert 40 <= n_sq <= len(xs) - 40


def test_fp_lex_parity(lib2):
    rng = random.Random(22)
    xs = [0, 1, 2, P - 1, P - 2, C.HALF, C.HALF + 1, C.HALF - 1] + [rng.randrange(P) for _ in range(200)]
    a = [[C.mont(x)] for x in xs]
    assert [bool(r[0]) for r in run2(lib2, F_LEX, 0, a)] == [O.fp_lex_largest(x) for x in xs]
    assert [int(r[0]) for r in run2(lib2, F_PARITY, 0, a)] == [x & 1 for x in xs]


@pytest.mark.parametrize("var", UN_VARS)
def test_fp_mont_conversions(lib2, var):
    xs = edge_and_random(200, P, 23)
    assert rows(run2(lib2, F_TO_MONT, var, [[x] for x in xs]), 1) == [[x * R % P] for x in xs]
    assert rows(run2(lib2, F_FROM_MONT, var, [[x] for x in xs]), 1) == [[x * RINV % P] for x in xs]


def test_fp_be48(lib2):
    rng = random.Random(24)
    xs = [0, 1, P - 1, P, P + 1, R - 1, 1 << 383, (1 << 381) - 1, 0x0102030405060708090A0B0C << 288]
    xs += [rng.randrange(R) for _ in range(100)] + [rng.randrange(P) for _ in range(100)]
    raw = np.frombuffer(b"".join(x.to_bytes(48, "big") for x in xs), np.uint8).view(np.uint32).reshape(-1, 12)
    out = run2(lib2, F_FROM_BE48, 0, raw)
    assert rows(out, 1) == [[x] for x in xs]
    assert [bool(r[12]) for r in out] == [x < P for x in xs]
    out = run2(lib2, F_TO_BE48, 0, [[x] for x in xs])
    assert [bytes(r.view(np.uint8)) for r in out] == [x.to_bytes(48, "big") for x in xs]


# ---- Fp2 --------------------------------------------------------------------------------
@pytest.mark.parametrize("var", BIN_VARS)
def test_fp2_add_sub_subadd(lib2, var):
    pairs = C.addsub_pairs()
    rng = random.Random(31)
    # coefficient pairs drawn independently: (a0, b0) and (a1, b1) are both edge pairs
    sel = [(p, rng.choice(pairs)) for p in pairs] + [(p, p) for p in pairs[:200]]
    xs = [[p[0], q[0]] for p, q in sel]
    ys = [[p[1], q[1]] for p, q in sel]
    ea, eb = alias(var, xs, ys)
    assert rows(run2(lib2, F2_ADD, var, xs, ys), 2) == [[(a[0] + b[0]) % P, (a[1] + b[1]) % P] for a, b in zip(ea, eb)]
    assert rows(run2(lib2, F2_SUB, var, xs, ys), 2) == [[(a[0] - b[0]) % P, (a[1] - b[1]) % P] for a, b in zip(ea, eb)]
    assert rows(run2(lib2, F2_SUBADD, var, xs, ys), 2) == [[(a[0] - b[0]) % P, (a[1] + b[1]) % P]
                                                          for a, b in zip(ea, eb)]


@pytest.mark.parametrize("var", UN_VARS)
def test_fp2_linear(lib2, var):
    """fp2_dbl and fp2_mul_xi feed the add/sub asm equal-valued operands (x.c0 == x.c1)."""
    vals = C.fp2_values(300, 32)
    xs = [list(v) for v in vals]
    assert rows(run2(lib2, F2_DBL, var, xs), 2) == [[2 * a % P, 2 * b % P] for a, b in vals]
    assert rows(run2(lib2, F2_NEG, var, xs), 2) == [[-a % P, -b % P] for a, b in vals]
    assert rows(run2(lib2, F2_CONJ, var, xs), 2) == [[a, -b % P] for a, b in vals]
    assert rows(run2(lib2, F2_MUL_XI, var, xs), 2) == [[(a - b) % P, (a + b) % P] for a, b in vals]
    assert rows(run2(lib2, F2_MUL3, var, xs), 2) == [[3 * a % P, 3 * b % P] for a, b in vals]


@pytest.mark.parametrize("var", BIN_VARS)
def test_fp2_mul_aliased(lib2, var):
    xs, ys = C.fp2_values(150, 33), list(reversed(C.fp2_values(150, 34)))
    ea, eb = alias(var, xs, ys)
    assert un2(run2(lib2, F2_MUL, var, m2(xs), m2(ys))) == [O.f2_mul(a, b) for a, b in zip(ea, eb)]


@pytest.mark.parametrize("var", UN_VARS)
def test_fp2_sqr_inv_mul_fp(lib2, var):
    xs = C.fp2_values(150, 35)
    assert un2(run2(lib2, F2_SQR, var, m2(xs))) == [O.f2_sqr(a) for a in xs]
    got = un2(run2(lib2, F2_INV, var, m2(xs)))
    for a, r in zip(xs, got):
        # a0^2 + a1^2 = 0 only for a = 0 (-1 is a non-residue); inv(0) = 0
        assert r == (O.f2_inv(a) if a != (0, 0) else (0, 0)), a
    ks = edge_and_random(len(xs) - len(EDGE), P, 36)
    got = un2(run2(lib2, F2_MUL_FP, var, m2(xs), [[C.mont(k)] for k in ks]))
    assert got == [O.f2_mul_fp(a, k) for a, k in zip(xs, ks)]


def test_fp2_sgn0_lex(lib2):
    xs = C.fp2_values(200, 37)
    xs += [(a, b) for a in (0, 1, C.HALF, C.HALF + 1, P - 1) for b in (0, 1, C.HALF, C.HALF + 1, P - 1)]
    assert [int(r[0]) for r in run2(lib2, F2_SGN0, 0, m2(xs))] == [O.f2_sgn0(a) for a in xs]
    assert [bool(r[0]) for r in run2(lib2, F2_LEX, 0, m2(xs))] == [O.f2_lex_largest(a) for a in xs]


@pytest.mark.parametrize("var", UN_VARS)
def test_fp2_sqrt(lib2, var):
    """All six outcomes of fp2_sqrt (tests/test_field_cases.py asserts the inputs reach each
    at least 8 times); either root is accepted."""
    xs = C.fp2_sqrt_inputs()
    out = run2(lib2, F2_SQRT, var, m2(xs))
    for a, r, row in zip(xs, un2(out), out):
        want = O.f2_is_square(a)
        assert bool(row[24]) == want, (C.fp2_sqrt_outcome(a), a)
        if want:
            assert O.f2_sqr(r) == a, (C.fp2_sqrt_outcome(a), a)


def test_fpw_kcombine(lib2):
    """t0 <- t0 - t1 mod pR, t2 <- t2 - t0 - t1 on double-width edge inputs (t0 < t1
    included); t2 >= t0 + t1 as in the Karatsuba product."""
    rng = random.Random(41)
    PR = P * R
    edge = [0, 1, PR - 1, PR - 2, P * P, (P - 1) ** 2, R - 1, R, R + 1, (1 << 704) - 1, 1 << 704, (R - 1) * (1 << 352),
            PR // 2, P, P - 1, (1 << 736) - 1]
    edge = [e % PR for e in edge]
    cases = [(a, b) for a in edge for b in edge] + [(rng.randrange(PR), rng.randrange(PR)) for _ in range(300)]
    t2 = []
    for i, (a, b) in enumerate(cases):
        room = (1 << 768) - 1 - a - b
        d = [0, 1, room, (1 << 384) - 1, rng.randrange(room + 1)][i % 5]
        t2.append(a + b + min(d, room))
    assert any(a < b for a, b in cases) and any(a > b for a, b in cases)
    a = np.concatenate([C.limbs([c[0] for c in cases], 24), C.limbs([c[1] for c in cases], 24)], axis=1)
    out = run2(lib2, FW_KCOMBINE, 0, a, C.limbs(t2, 24))
    assert C.ints(out[:, :24]) == [(x - y) % PR for x, y in cases]
    assert C.ints(out[:, 24:]) == [t - x - y for (x, y), t in zip(cases, t2)]


# ---- Fp6 --------------------------------------------------------------------------------
@pytest.mark.parametrize("var", BIN_VARS)
def test_fp6_mul(lib2, var):
    xs, ys = C.f6_values(80, 51), list(reversed(C.f6_values(80, 52)))
    ea, eb = alias(var, xs, ys)
    assert un6(run2(lib2, F6_MUL, var, m6(xs), m6(ys))) == [O.f6_mul(a, b) for a, b in zip(ea, eb)]


@pytest.mark.parametrize("var", UN_VARS)
def test_fp6_sparse_and_inv(lib2, var):
    """fp6_mul_01 / _1 / _12 against the full product with the embedded element."""
    xs = C.f6_values(80, 53)
    b0 = C.fp2_values(len(xs) - 16, 54)
    b1 = list(reversed(C.fp2_values(len(xs) - 16, 55)))
    z = O.F2_ZERO
    both = [[C.mont(c) for c in p + q] for p, q in zip(b0, b1)]
    assert un6(run2(lib2, F6_MUL_01, var, m6(xs), both)) == [O.f6_mul(a, (p, q, z)) for a, p, q in zip(xs, b0, b1)]
    assert un6(run2(lib2, F6_MUL_1, var, m6(xs), m2(b1))) == [O.f6_mul(a, (z, q, z)) for a, q in zip(xs, b1)]
    assert un6(run2(lib2, F6_MUL_12, var, m6(xs), both)) == [O.f6_mul(a, (z, p, q)) for a, p, q in zip(xs, b0, b1)]
    assert un6(run2(lib2, F6_MUL_V, var, m6(xs))) == [O.f6_mul_v(a) for a in xs]
    nz = [a for a in xs if a != O.F6_ZERO]
    assert un6(run2(lib2, F6_INV, var, m6(nz))) == [O.f6_inv(a) for a in nz]


# ---- Fp12 -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def f12_cases():
    return C.f12_values(100, 61), list(reversed(C.f12_values(100, 62)))


@pytest.mark.parametrize("var", BIN_VARS)
def test_fp12_mul(lib2, f12_cases, var):
    xs, ys = f12_cases
    ea, eb = alias(var, xs, ys)
    assert un12(run2(lib2, F12_MUL, var, m12(xs), m12(ys))) == [O.f12_mul(a, b) for a, b in zip(ea, eb)]


@pytest.mark.parametrize("var", UN_VARS)
def test_fp12_sqr_conj_inv(lib2, f12_cases, var):
    xs = f12_cases[0]
    assert un12(run2(lib2, F12_SQR, var, m12(xs))) == [O.f12_sqr(a) for a in xs]
    assert un12(run2(lib2, F12_CONJ, var, m12(xs))) == [O.f12_conj(a) for a in xs]
    nz = [a for a in xs if any(C.f12_flat(a))]
    assert un12(run2(lib2, F12_INV, var, m12(nz))) == [O.f12_inv(a) for a in nz]


@pytest.mark.parametrize("var", UN_VARS)
def test_fp12_sparse_products(lib2, f12_cases, var):
    """fp12_mul_line, and line_mul_line followed by fp12_mul_by_sparse2, against the full
    O.f12_mul with the embedded lines; line coefficients include 0 and p - 1."""
    xs = f12_cases[0]
    n = len(xs) - 16
    ls = [C.fp2_values(n, 63 + j) for j in range(6)]
    ls = [l if j % 2 == 0 else list(reversed(l)) for j, l in enumerate(ls)]
    line3 = [[C.mont(c) for c in a + b + c4] for a, b, c4 in zip(ls[0], ls[1], ls[2])]
    got = un12(run2(lib2, F12_MUL_LINE, var, m12(xs), line3))
    assert got == [O.f12_mul(f, C.embed_line(a, b, c4)) for f, a, b, c4 in zip(xs, ls[0], ls[1], ls[2])]
    line6 = [[C.mont(c) for l in six for c in l] for six in zip(*ls)]
    got = un12(run2(lib2, F12_LINE_LINE, var, m12(xs), line6))
    want = [O.f12_mul(f, O.f12_mul(C.embed_line(*six[:3]), C.embed_line(*six[3:]))) for f, six in zip(xs, zip(*ls))]
    assert got == want


@pytest.mark.parametrize("var", UN_VARS)
def test_fp12_frobenius(lib2, f12_cases, var):
    """Against the coefficient formula of tests/field_cases.py (constants from O.f2_pow),
    which is itself checked against O.f12_pow(a, p^k) on two elements per k; O.f12_pow on
    every case would take about a minute."""
    xs = f12_cases[0]
    for k, op in ((1, F12_FROB1), (2, F12_FROB2), (3, F12_FROB3)):
        if var == 0:
            for a in (xs[2], xs[-1]):
                assert C.f12_frob(a, k) == O.f12_pow(a, P ** k)
        assert un12(run2(lib2, op, var, m12(xs))) == [C.f12_frob(a, k) for a in xs]


@pytest.mark.parametrize("var", UN_VARS)
def test_fp12_cyc_sqr(lib2, f12_cases, var):
    """Granger-Scott squaring on inputs made cyclotomic in Python: a -> a^((p^6-1)(p^2+1))."""
    xs = [C.f12_cyclotomic(a) for a in f12_cases[0] if any(C.f12_flat(a))]
    assert O.F12_ONE in xs
    assert un12(run2(lib2, F12_CYC_SQR, var, m12(xs))) == [O.f12_sqr(a) for a in xs]


def test_fp12_is_one(lib2, f12_cases):
    xs = f12_cases[0] + [O.F12_ONE]
    rng = random.Random(71)
    for pos in range(12):  # one, with one coefficient disturbed
        c = C.f12_flat(O.F12_ONE)
        c[pos] = (c[pos] + rng.choice([1, P - 1])) % P
        xs.append(C.f12_unflat(c))
    assert [bool(r[0]) for r in run2(lib2, F12_IS_ONE, 0, m12(xs))] == [a == O.F12_ONE for a in xs]
