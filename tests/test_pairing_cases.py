"""CPU checks of the case lists behind tests/test_gpu_pairing.py: the inputs really reach
every extreme, scale and aliasing form the GPU tests claim to cover, and the Python
evaluation of the generated programs (the GPU test's expectation) agrees with the oracle."""
import pytest

from oracle import bls12_381 as O
from tests import field_cases as C
from tests import pairing_cases as K
from tests import wc12_helper as W

P = O.P


@pytest.mark.parametrize("name", K.PROGRAMS)
def test_every_operand_form_has_both_extremes(name):
    """For each x_k and y_k of each program one case drives the signed sum to
    +(positive weight)(p - 1) and another to -(negative weight)(p - 1).  A program that
    gains a form the cases do not reach fails here."""
    prog, _ = W.program(name)
    cases = K.extreme_cases(name)
    assert len(prog.prods) == 0 or cases
    for k, (x, y) in enumerate(prog.prods):
        for which, form in (("x", x), ("y", y)):
            pos, neg = K.form_weights(form)
            assert 1 <= pos + neg <= W.G.CHUNK, (name, k, which)
            sums = {K.form_value(form, a, b) for a, b in cases}
            assert pos * (P - 1) in sums, (name, k, which, "max")
            assert -neg * (P - 1) in sums, (name, k, which, "min")
    for a, b in cases:
        assert all(0 <= v < P for v in a + b)
    assert len(set((tuple(a), tuple(b)) for a, b in cases)) == len(cases)


def test_programs_are_the_table_order():
    assert K.PROGRAMS == ("MUL", "SQR", "CYC", "LINE", "FROB1", "FROB2", "FROB3", "CONJ")
    assert set(K.FORMS) == set(K.PROGRAMS)


def test_aliasing_forms_present():
    assert set(K.FORMS["MUL"]) == {0, 1, 2, 3}           # distinct, dst == a, dst == b, a == b
    for name in K.PROGRAMS:
        assert {0, 1} <= set(K.FORMS[name]), name        # distinct and dst == a
    for name in K.FROBS:
        assert 4 in K.FORMS[name]                        # b from the host: the y forms' extremes
    for name in K.UNARY:
        assert all(a == b for a, b in K.apply_cases(name))


def test_edge_set_holds_the_field_cases():
    for name in K.PROGRAMS:
        a_side = [tuple(a) for a, _ in K.edge_cases(name)]
        assert (0,) * 12 in a_side and (1,) + (0,) * 11 in a_side and (P - 1,) * 12 in a_side
        for pos in range(12):
            assert any(a[pos] == 1 and sum(a) == 1 for a in a_side), (name, pos)
            assert any(a[pos] == P - 1 and sum(a) == P - 1 for a in a_side), (name, pos)
    for _, b in K.apply_cases("LINE"):
        assert all(b[6:]), "slots 6..11 of a line operand hold non-zero junk"


@pytest.mark.parametrize("name", ["MUL", "SQR", "LINE", "FROB1", "FROB2", "FROB3", "CONJ"])
def test_program_evaluation_agrees_with_oracle_on_extremes(name):
    cases = K.extreme_cases(name) + K.edge_cases(name)[:8]
    for a, b in cases:
        if name in K.FROBS:
            b = K.gammas(K.FROBS[name])
        assert W.run_named(name, a, b) == K.oracle_apply(name, a, b), (name, a, b)


def test_cyc_is_a_squaring_on_cyclotomic_inputs():
    for a in K.exp_x_inputs()[:3]:
        assert W.run_named("CYC", C.f12_flat(a), C.f12_flat(a)) == C.f12_flat(O.f12_sqr(a))


def test_step_cases_hold_every_scale_and_coordinate():
    cases = K.step_cases()
    pts = K.e2_points()
    assert len(pts) == 5 and all(O.E2.on_curve(t) for t in pts)
    zs = K.step_scales()
    assert zs[0] == (1, 0) and zs[1] == (P - 1, 0) and len(set(zs)) == 4
    assert all(z[0] and z[1] for z in zs[2:])
    xs = set(K.step_p_coords())
    assert {0, 1, P - 1} < xs and len(xs) == 4
    for t in pts:
        for z in zs:
            assert {(xp, yp) for tt, zz, _, xp, yp in cases if tt == t and zz == z} == {(a, b) for a in xs for b in xs}
    for t, z, q, _, _ in cases:
        assert q != t and q != O.E2.neg(t) and O.E2.on_curve(q)
        assert K.unproj(*K.proj(t, z)) == t


def test_proportional_rejects_a_wrong_line():
    t, p = K.e2_points()[1], (5, 7)
    c = K.oracle_line(K.tangent_slope(t), t, p)
    k = (3, 9)
    scaled = tuple(O.f2_mul(x, k) for x in c)
    assert K.proportional(scaled, c)
    assert not K.proportional((scaled[0], scaled[1], O.f2_add(scaled[2], (1, 0))), c)
    assert not K.proportional((O.F2_ZERO,) * 3, c)
    # the tangent at T is the chord's limit: both oracle lines vanish at the points they join
    q = K.e2_points()[2]
    lam = K.chord_slope(t, q)
    assert O.f2_sub(O.f2_mul(lam, O.f2_sub(q[0], t[0])), O.f2_sub(q[1], t[1])) == O.F2_ZERO


def test_pairs_are_distinct_and_hold_the_miller_cases():
    prs = K.pairs()
    assert len(prs) == max(K.LINE_PAIR_COUNTS) == 65 and len(set(prs)) == 65
    assert all(O.E1.on_curve(p) and O.E2.on_curve(q) for p, q in prs)
    assert prs[0] == (O.G1, O.G2) and prs[1] == (O.E1.neg(O.G1), O.G2)
    assert K.MAX_MILLER_PAIRS == 8
    sched = K.loop_schedule()
    assert len(sched) == K.N_LINES and sched.count("dbl") == 63 and sched.count("add") == 5 and sched[0] == "dbl"


def test_final_exp_inputs_within_cap_and_subfield_inputs_map_to_one():
    cases = K.final_exp_inputs()
    names = [n for n, _, _ in cases]
    assert len(cases) <= K.MAX_FINAL_EXP_INPUTS == 24 and len(set(names)) == len(names)
    assert len(set(f for _, f, _ in cases)) == len(cases)
    for want in ("one", "minus_one", "fp2", "fp6", "all_p_minus_1", "miller_0", "miller_4", "miller_product", "gt"):
        assert want in names
    assert sum(n.startswith("unit_") for n in names) == 11 and sum(n.startswith("random_") for n in names) == 4
    by = {n: f for n, f, _ in cases}
    assert C.f12_flat(by["one"]) == [1] + [0] * 11 and C.f12_flat(by["minus_one"]) == [P - 1] + [0] * 11
    assert not any(C.f12_flat(by["fp2"])[2:]) and all(C.f12_flat(by["fp2"])[:2])
    assert not any(C.f12_flat(by["fp6"])[6:]) and all(C.f12_flat(by["fp6"])[:6])
    for name, f, to_one in cases:
        if to_one:
            assert O.f12_is_one(O.final_exp(f)), name
    assert len(K.exp_x_inputs()) == 9 and K.exp_x_inputs()[-1] == O.F12_ONE
    assert len(K.not_one_inputs()) == 12 and not any(O.f12_is_one(f) for f in K.not_one_inputs())
