"""Inputs and Python-integer expectations shared by tests/test_gpu_field.py (GPU)
and tests/test_field_cases.py (CPU: the case lists really hold what they claim).
Field elements travel as raw little-endian 32-bit limbs; a "raw" value below is
the integer the limbs spell (the Montgomery representative where the routine
takes one), a "canonical" value is raw * R^-1 mod p."""
import random

import numpy as np

from oracle import bls12_381 as O

P = O.P
R = 1 << 384
RINV = pow(R, -1, P)
HALF = (P - 1) // 2

EDGE = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (1 << 381) - 1, (1 << 352) - 1, 0xFFFFFFFF, 1 << 380]


def limbs(vals, n=12):
    out = np.zeros((len(vals), n), np.uint32)
    for i, v in enumerate(vals):
        assert 0 <= v < 1 << (32 * n)
        for j in range(n):
            out[i, j] = (v >> (32 * j)) & 0xFFFFFFFF
    return out


def ints(arr):
    return [sum(int(x) << (32 * j) for j, x in enumerate(row)) for row in arr]


def mont(x):
    return x * R % P


def unmont(x):
    return x * RINV % P


def addsub_pairs():
    """(a, b) with a, b < p: the sums and differences next to the reduction
    threshold, 0 and p - 1 on either side, a = b, carries and borrows through all
    twelve limbs, EDGE x EDGE and random values."""
    rng = random.Random(101)
    base = [v % P for v in EDGE] + [(P + 1) // 2, 1 << 352, (1 << 352) + 1, (1 << 320) - 1, (1 << 32) - 1, 1 << 32,
                                    (1 << 380) - 1, P - (1 << 352), P - (1 << 32)]
    base += [rng.randrange(P) for _ in range(20)]
    pairs = []
    for a in base:
        for b in (P - 1 - a, P - a, P + 1 - a, a + 1, a, a - 1, 0, P - 1):
            if 0 <= b < P:
                pairs.append((a, b))
                pairs.append((b, a))
    # ripples: 2^352 - 1 plus 1, 2^352 minus 1, all-ones low limbs plus / minus one
    for k in range(1, 12):
        ones = (1 << (32 * k)) - 1
        pairs += [(ones, 1), (1, ones), (1 << (32 * k), 1), (ones, ones), (0, ones), (ones, P - 1)]
    pairs += [(a % P, b % P) for a in EDGE for b in EDGE]
    pairs += [(rng.randrange(P), rng.randrange(P)) for _ in range(300)]
    return pairs


def inv_inputs():
    """A GPU-sized cut of the tests/test_fp_inv.py list (raw values the GCD sees)."""
    rng = random.Random(2024)
    xs = [0, 1, 2, 3, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2]
    xs += [1 << k for k in range(0, 381)]
    xs += [(1 << k) - 1 for k in range(1, 381)]
    xs += [P - (1 << k) for k in range(0, 380)]
    xs += [int("5" * 95, 16) % P, int("a" * 95, 16) % P, int("f" * 95, 16) % P]
    xs += [rng.randrange(P) for _ in range(300)]
    xs += [rng.randrange(1 << rng.randrange(1, 381)) for _ in range(100)]
    return xs


def fp2_values(k, seed):
    """Fp2 elements with each coefficient drawn independently from EDGE and random
    values, so that c0 = c1, c0 = 0 and c1 = 0 all occur."""
    rng = random.Random(seed)
    pool = [v % P for v in EDGE] + [rng.randrange(P) for _ in range(6)]
    vals = [(a, b) for a in (0, 1, P - 1, pool[-1]) for b in (0, 1, P - 1, pool[-1])]
    vals += [(rng.choice(pool), rng.choice(pool)) for _ in range(k)]
    return vals


# ---- fp2_sqrt: the six outcomes of lodestar_amd/csrc/bls_field.h ----------------
SQRT_OUTCOMES = ("zero", "a1_zero_qr", "a1_zero_nqr", "general_t_qr", "general_t_nqr", "not_square")


def fp2_sqrt_outcome(a):
    """Replays the branch conditions of fp2_sqrt on canonical (a0, a1)."""
    a0, a1 = a
    if a1 == 0:
        if a0 == 0:
            return "zero"
        return "a1_zero_qr" if pow(a0, (P - 1) // 2, P) == 1 else "a1_zero_nqr"
    n = (a0 * a0 + a1 * a1) % P
    s = pow(n, (P + 1) // 4, P)
    if s * s % P != n:
        return "not_square"
    t = (a0 + s) * ((P + 1) // 2) % P
    x0 = pow(t, (P + 1) // 4, P)
    return "general_t_qr" if x0 * x0 % P == t else "general_t_nqr"


def fp2_sqrt_inputs():
    rng = random.Random(77)
    vals = [(0, 0)] * 8
    ks = [1, 2, 3, P - 1, (P - 1) // 2] + [rng.randrange(1, P) for _ in range(8)]
    vals += [(k * k % P, 0) for k in ks]            # a1 = 0, a0 a residue
    vals += [((-k * k) % P, 0) for k in ks]         # a1 = 0, a0 a non-residue (-1 is one: p = 3 mod 4)
    vals += [(0, 1), (0, P - 1), (1, 1), (P - 1, P - 1), (1, P - 1), (0, 4), (4, 4)]
    for _ in range(60):                             # squares of random elements: the two general cases
        z = (rng.randrange(P), rng.randrange(1, P))
        vals.append(O.f2_sqr(z))
    vals += [(rng.randrange(P), rng.randrange(P)) for _ in range(200)]
    return vals


# ---- Fp6 / Fp12 ---------------------------------------------------------------
def f12_flat(a):
    """Fp12 tuple -> the 12 Fp coefficients in the order of struct fp12."""
    return [c for f6 in a for f2 in f6 for c in f2]


def f12_unflat(c):
    return tuple(tuple((c[6 * i + 2 * j], c[6 * i + 2 * j + 1]) for j in range(3)) for i in range(2))


def f6_flat(a):
    return [c for f2 in a for c in f2]


def f6_unflat(c):
    return tuple((c[2 * j], c[2 * j + 1]) for j in range(3))


def f12_values(k, seed):
    """0, 1, a single non-zero coefficient at each of the twelve positions (1 and
    p - 1), all coefficients p - 1, and k random elements."""
    rng = random.Random(seed)
    vals = [[0] * 12, [1] + [0] * 11, [P - 1] * 12]
    for pos in range(12):
        for v in (1, P - 1, rng.randrange(P)):
            c = [0] * 12
            c[pos] = v
            vals.append(c)
    vals += [[rng.randrange(P) for _ in range(12)] for _ in range(k)]
    return [f12_unflat(c) for c in vals]


def f6_values(k, seed):
    rng = random.Random(seed)
    vals = [[0] * 6, [1] + [0] * 5, [P - 1] * 6]
    for pos in range(6):
        for v in (1, P - 1):
            c = [0] * 6
            c[pos] = v
            vals.append(c)
    vals += [[rng.randrange(P) for _ in range(6)] for _ in range(k)]
    return [f6_unflat(c) for c in vals]


_GAMMA = {}


def f12_frob(a, k):
    """a^(p^k) by the coefficient formula: the coefficient of w^e (e = 2j + i for
    c_i.c_j) is conjugated k times and multiplied by xi^(e (p^k - 1) / 6).  The
    constants come from O.f2_pow here, not from the library's tables."""
    if k not in _GAMMA:
        _GAMMA[k] = [O.f2_pow((1, 1), e * (P ** k - 1) // 6) for e in range(6)]
    g = _GAMMA[k]
    out = []
    for i in range(2):
        row = []
        for j in range(3):
            x = a[i][j]
            if k & 1:
                x = O.f2_conj(x)
            row.append(O.f2_mul(x, g[2 * j + i]))
        out.append(tuple(row))
    return tuple(out)


def f12_cyclotomic(a):
    """a^((p^6 - 1)(p^2 + 1)), an element of the cyclotomic subgroup (a != 0)."""
    b = O.f12_mul(O.f12_conj(a), O.f12_inv(a))
    return O.f12_mul(f12_frob(b, 2), b)


def embed_line(l0, l1, l4):
    """(l0 + l1 v) + (l4 v) w as a full Fp12 element."""
    return ((l0, l1, O.F2_ZERO), (O.F2_ZERO, l4, O.F2_ZERO))
