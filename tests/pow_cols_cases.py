"""Inputs and Python-integer expectations shared by tests/test_fp_pow_cols.py (host build) and
tests/test_gpu_pow_cols.py (gfx950 build) of lodestar_amd/csrc/bls_fp_pow.h: a^((p-3)/4) on 13
digits of 30 bits, Montgomery radix 2^390 inside, 2^384 at its boundary."""
import random

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 1 << 384
RINV = pow(R, -1, P)
R390 = 1 << 390
PINV390 = pow(P, -1, R390)
E = (P - 3) // 4
M30 = (1 << 30) - 1


def _canonical():
    rng = random.Random(20)
    vals = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, 1 << 380]
    # limbs of all ones below p: eleven whole limbs, and those under the top bits of p
    vals += [(1 << 352) - 1, (1 << 380) | ((1 << 352) - 1)]
    # 30-bit digits all 2^30 - 1: twelve whole digits, and with the top digit as full as p allows
    vals += [(1 << 360) - 1, (1 << 380) - 1]
    # one off each 2^(30 k) boundary
    for k in range(1, 13):
        vals += [(1 << (30 * k)) - 1, 1 << (30 * k), (1 << (30 * k)) + 1]
    vals += [rng.randrange(P) for _ in range(400)]
    assert all(0 <= v < P for v in vals) and len(vals) <= 512
    return vals


def _resident():
    """Operands of the in-chain primitives: up to the documented bound, 2p (digits < 2^30)."""
    rng = random.Random(21)
    vals = _canonical()[:47]
    vals += [P, P + 1, 2 * P - 1, 2 * P - 2, (1 << 381) - 1, 1 << 381, (1 << 381) + 1, (3 * P) // 2]
    vals += [rng.randrange(2 * P) for _ in range(400)]
    assert all(0 <= v < 2 * P for v in vals) and len(vals) <= 512
    return vals


CANONICAL = _canonical()
RESIDENT = _resident()
# second operands of the resident product: the same values in another order
RESIDENT_B = [RESIDENT[(7 * k + 3) % len(RESIDENT)] for k in range(len(RESIDENT))]


def digits(v):
    return [(v >> (30 * i)) & M30 for i in range(13)]


def from_digits(d):
    return sum(int(x) << (30 * i) for i, x in enumerate(d))


def limbs(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)]


def from_limbs(a):
    return sum(int(x) << (32 * i) for i, x in enumerate(a))


def mont390(x):
    """The exact value a Montgomery reduction by 2^390 returns for the product x: (x + m p) / 2^390."""
    m = (-x * PINV390) % R390
    return (x + m * P) >> 390


def pow_expected(v):
    """fp_pow_p34 on the 12-limb Montgomery representative v = a 2^384: a^((p-3)/4) 2^384 mod p."""
    return pow(v * RINV % P, E, P) * R % P


def window_exponent(win):
    """The exponent a window program (bls_constants.h LB_P34_WIN) encodes."""
    e = 2 * (win[0] & 15) + 1
    for st in win[1:]:
        e <<= st >> 4
        if st & 15 <= 3:
            e += 2 * (st & 15) + 1
    return e
