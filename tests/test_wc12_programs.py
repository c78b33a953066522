"""The wave-cooperative Fp12 programs (lodestar_amd/csrc/gen_wc12.py: K parallel
Fp products + linear combinations per operation) evaluated on random inputs
against the oracle's Fp12 arithmetic.  CPU only: this pins the tables the
GPU's k_tail kernel executes."""
import random

import pytest

from oracle import bls12_381 as O
from tests.wc12_helper import G, flat, run, unflat

P = O.P


def rnd12(r):
    return [r.randrange(P) for _ in range(12)]


@pytest.fixture(scope="module")
def rng():
    return random.Random(2024)


def test_mul(rng):
    for _ in range(3):
        a, b = rnd12(rng), rnd12(rng)
        assert run(G.op_mul, a, b) == flat(O.f12_mul(unflat(a), unflat(b)))


def test_sqr(rng):
    a = rnd12(rng)
    assert run(G.op_sqr, a, a) == flat(O.f12_mul(unflat(a), unflat(a)))


def test_cyclotomic_sqr(rng):
    f = unflat(rnd12(rng))
    f = O.f12_mul(O.f12_conj(f), O.f12_inv(f))          # ^(p^6 - 1)
    f = O.f12_mul(O.f12_pow(f, P * P), f)               # ^(p^2 + 1): cyclotomic
    a = flat(f)
    assert run(G.op_cyc, a, a) == flat(O.f12_mul(f, f))


def test_line(rng):
    a = rnd12(rng)
    l0, l1, l4 = [(rng.randrange(P), rng.randrange(P)) for _ in range(3)]
    b = [l0[0], l0[1], l1[0], l1[1], l4[0], l4[1]] + [0] * 6
    line = ((l0, l1, O.F2_ZERO), (O.F2_ZERO, l4, O.F2_ZERO))
    assert run(G.op_line, a, b) == flat(O.f12_mul(unflat(a), line))


@pytest.mark.parametrize("k", [1, 2, 3])
def test_frobenius(rng, k):
    a = rnd12(rng)
    xi = (1, 1)
    gam = [O.f2_pow(xi, e * (P ** k - 1) // 6) for e in range(6)]
    b = [c for g in gam for c in g]
    assert run({1: lambda: G.op_frob(1), 2: lambda: G.op_frob(2), 3: lambda: G.op_frob(3)}[k], a, b) == \
        flat(O.f12_pow(unflat(a), P ** k))


def test_conj(rng):
    a = rnd12(rng)
    assert run(G.op_conj, a, a) == flat(O.f12_conj(unflat(a)))


def test_no_all_negative_run_of_full_weight():
    """lz_sum (bls_wc12.h) reduces [0, w p] for w < 8 and [0, 8p) for w = 8: a form or an
    output chunk of weight 8 whose coefficients are all negative would reach 8p on zero terms."""
    seen = 0
    for name, fn in G.OPS:
        prog, out = fn()
        for x, y in prog.prods:
            for form in (x, y):
                assert not G.all_negative_full(G.enc_terms(form, {"A", "B"})), name
        for o in out.flat():
            for ch in G.chunks(G.enc_terms(o, {"A", "B", "P"})):
                assert sum(abs(c) for c, _ in ch) <= G.CHUNK and not G.all_negative_full(ch), name
                seen += all(c < 0 for c, _ in ch)
    assert seen  # all-negative runs exist (the conjugate's outputs): the closed upper end matters
    assert G.all_negative_full([(-3, 0), (-5, 1)]) and not G.all_negative_full([(-3, 0), (5, 1)])
