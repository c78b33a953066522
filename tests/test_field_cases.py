"""CPU checks of the case lists behind tests/test_gpu_field.py: the inputs really reach
every branch and edge the GPU tests claim to cover."""
from oracle import bls12_381 as O
from tests import field_cases as C

P = C.P


def test_fp2_sqrt_inputs_reach_all_six_outcomes():
    xs = C.fp2_sqrt_inputs()
    count = {k: 0 for k in C.SQRT_OUTCOMES}
    for a in xs:
        kind = C.fp2_sqrt_outcome(a)
        count[kind] += 1
        assert (kind != "not_square") == O.f2_is_square(a), a
    assert all(v >= 8 for v in count.values()), count
    # the non-square share of the random draws is near one half
    assert 0.25 < count["not_square"] / len(xs) < 0.6, count


def test_addsub_pairs_hold_the_edges():
    pairs = C.addsub_pairs()
    assert all(0 <= a < P and 0 <= b < P for a, b in pairs)
    sums = {a + b for a, b in pairs}
    diffs = {a - b for a, b in pairs}
    assert {P - 1, P, P + 1} <= sums and {-1, 0, 1} <= diffs
    assert ((1 << 352) - 1, 1) in pairs and (1 << 352, 1) in pairs
    assert any(a == 0 for a, _ in pairs) and any(b == P - 1 for _, b in pairs)


def test_fp2_values_cover_equal_and_zero_coefficients():
    vals = C.fp2_values(300, 32)
    assert any(a == b != 0 for a, b in vals) and any(a == 0 != b for a, b in vals) and any(b == 0 != a for a, b in vals)


def test_frobenius_formula_and_cyclotomic_inputs():
    a = C.f12_values(1, 5)[-1]
    assert C.f12_frob(a, 1) == O.f12_pow(a, P)
    c = C.f12_cyclotomic(a)
    # cyclotomic: c^(p^4 - p^2 + 1) = 1  <=>  frob4(c) * c = frob2(c)
    assert O.f12_mul(C.f12_frob(C.f12_frob(c, 2), 2), c) == C.f12_frob(c, 2)
