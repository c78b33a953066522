"""GPU checks of the pairing layer, one primitive at a time: the Miller steps and the
stored-line Miller loop of lodestar_amd/csrc/bls_pairing.h, miller_loop, final_exp, and the
wave-cooperative Fp12 of bls_wc12.h (wc_apply over the eight generated programs, wc_exp_x,
wc_final_exp, wc_miller_from_lines, wc_is_one) that every verification's tail runs on.

Values go in and come out as raw Montgomery limbs.  An expected value is the canonical
Montgomery form computed here, compared with the INTEGER the limbs spell, not its residue:
an output of v + p fails (fp_eq and wc_is_one depend on canonical outputs).  The HIP side is
tests/native/pairing_selftest.hip + pairing_wc_selftest.hip (built by build(); test-only);
the case lists are tests/pairing_cases.py, checked on the CPU by tests/test_pairing_cases.py."""
import ctypes
import os

import numpy as np
import pytest

from oracle import bls12_381 as O
from tests import field_cases as C
from tests import pairing_cases as K
from tests import wc12_helper as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (LB_PAIRING_SELFTEST: another build of the same self-test)
LIB = os.environ.get("LB_PAIRING_SELFTEST") or os.path.join(ROOT, "tests", "native", "libpairing_selftest.so")
P = O.P

pytestmark = pytest.mark.gpu

P_DBL, P_ADD = 0, 1
P_MILLER, P_FINAL_EXP, P_EXP_X = 10, 11, 12
L_LINES, L_LINES_QMEM = 0, 1
W_APPLY, W_SLOTS, W_IS_ONE, W_EXP_X, W_FINAL_EXP = range(5)
LINE_WORDS = 72
SENTINEL = 0xA5C3F00D
GUARD = 4096


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("tests/native/libpairing_selftest.so missing: run __graft_entry__.build()")
    L = ctypes.CDLL(LIB)
    vp, u32, i = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.lbt_pairing_op_widths.argtypes = [i, vp]
    L.lbt_pairing_op.argtypes = [i, i, u32, vp, vp, vp]
    L.lbt_pairing_lines_widths.argtypes = [vp]
    L.lbt_pairing_lines.argtypes = [i, u32, u32, vp, vp]
    L.lbt_pairing_line_get.argtypes = [u32, vp, vp]
    L.lbt_wc_op_widths.argtypes = [i, vp]
    L.lbt_wc_op.argtypes = [i, i, i, u32, vp, vp, vp]
    L.lbt_wc_miller.argtypes = [u32, vp, u32, vp, vp]
    return L


# ---- conversions -------------------------------------------------------------------------
def words(rows):
    """rows of canonical Fp values -> uint32 (n, 12 * len(row)) of Montgomery limbs."""
    return np.stack([C.limbs([C.mont(v) for v in r], 12).reshape(-1) for r in rows])


def raw(row):
    """uint32 words -> the integers the limbs spell (Montgomery representatives, unreduced)."""
    return C.ints(np.asarray(row).reshape(-1, 12))


def mont_all(vals):
    return [C.mont(v) for v in vals]


def fp2s(row):
    """Raw words -> Fp2 values; the limbs must spell canonical values."""
    r = raw(row)
    assert all(v < P for v in r), "non-canonical limbs"
    v = [C.unmont(x) for x in r]
    return [(v[2 * k], v[2 * k + 1]) for k in range(len(v) // 2)]


def f2c(*vals):
    return [c for v in vals for c in v]


def run1(lib, op, var, a, b=None):
    w = (ctypes.c_uint32 * 3)()
    assert lib.lbt_pairing_op_widths(op, w) == 0, op
    a = np.ascontiguousarray(a, np.uint32)
    n = a.shape[0]
    assert a.shape == (n, w[0]), (a.shape, w[0])
    bp = None
    if w[1]:
        b = np.ascontiguousarray(b, np.uint32)
        assert b.shape == (n, w[1]), (b.shape, w[1])
        bp = b.ctypes.data
    out = np.zeros((n, w[2]), np.uint32)
    rc = lib.lbt_pairing_op(op, var, n, a.ctypes.data, bp, out.ctypes.data)
    assert rc == 0, rc
    return out


def runw(lib, op, wop, var, a, b=None):
    """-> (n x 144 words, n flags)"""
    w = (ctypes.c_uint32 * 3)()
    assert lib.lbt_wc_op_widths(op, w) == 0, op
    a = np.ascontiguousarray(a, np.uint32)
    n = a.shape[0]
    assert a.shape == (n, w[0]), (a.shape, w[0])
    bp = None
    if w[1]:
        b = np.ascontiguousarray(b, np.uint32)
        assert b.shape == (n, w[1]), (b.shape, w[1])
        bp = b.ctypes.data
    out = np.zeros((n, w[2]), np.uint32)
    rc = lib.lbt_wc_op(op, wop, var, n, a.ctypes.data, bp, out.ctypes.data)
    assert rc == 0, rc
    return out[:, :144], out[:, 144]


def pq_words(prs, p_inf=(), q_inf=()):
    """x | y | inf of P, x | y | inf of Q per pair; an infinite point carries junk."""
    rows = []
    junk = np.full(48, 0xFFFFFFFF, np.uint32)
    for i, (p, q) in enumerate(prs):
        pw = junk[:24] if i in p_inf else words([list(p)])[0]
        qw = junk if i in q_inf else words([f2c(*q)])[0]
        rows.append(np.concatenate([pw, [1 if i in p_inf else 0], qw, [1 if i in q_inf else 0]]).astype(np.uint32))
    return np.stack(rows)


def run_lines(lib, var, prs, **inf):
    """-> (line array of 68 * 72 * n words, the guard words on both sides)"""
    n = len(prs)
    pq = pq_words(prs, **inf)
    w = (ctypes.c_uint32 * 2)()
    assert lib.lbt_pairing_lines_widths(w) == 0 and pq.shape == (n, w[0]) and w[1] == K.N_LINES * LINE_WORDS
    buf = np.full(2 * GUARD + w[1] * n, SENTINEL, np.uint32)
    rc = lib.lbt_pairing_lines(var, n, GUARD, pq.ctypes.data, buf.ctypes.data)
    assert rc == 0, rc
    return buf[GUARD:-GUARD], np.concatenate([buf[:GUARD], buf[-GUARD:]])


# ---- A. Miller steps ---------------------------------------------------------------------
def step_inputs():
    cases = K.step_cases()
    a = words([f2c(*K.proj(t, z)) + [xp, yp] for t, z, _, xp, yp in cases])
    b = words([f2c(*q) for _, _, q, _, _ in cases])
    return cases, a, b


def check_step(row, want_t, want_line, what):
    X, Y, Z, l0, l1, l4 = fp2s(row)
    assert not O.f2_is_zero(Z), what
    assert K.unproj(X, Y, Z) == want_t, what
    assert K.proportional((l0, l1, l4), want_line), what


def test_miller_dbl_step(lib):
    """T' = 2T against E2.double; (l0 : l1 : l4) proportional to the oracle's tangent line.
    miller_dbl_step_put (the line stored through a one-pair buffer before the point update)
    gives the same words bit for bit."""
    cases, a, _ = step_inputs()
    out = run1(lib, P_DBL, 0, a)
    dbl = {t: (O.E2.double(t), K.tangent_slope(t)) for t in K.e2_points()}
    for (t, z, _, xp, yp), row in zip(cases, out):
        check_step(row, dbl[t][0], K.oracle_line(dbl[t][1], t, (xp, yp)), (t, z, xp, yp))
    assert np.array_equal(run1(lib, P_DBL, 1, a), out)


def test_miller_add_step(lib):
    """T' = T + Q against E2.add; the chord through T and Q against the oracle's line."""
    cases, a, b = step_inputs()
    out = run1(lib, P_ADD, 0, a, b)
    memo = {}
    for (t, z, q, xp, yp), row in zip(cases, out):
        if (t, q) not in memo:
            memo[(t, q)] = (O.E2.add(t, q), K.chord_slope(t, q))
        check_step(row, memo[(t, q)][0], K.oracle_line(memo[(t, q)][1], t, (xp, yp)), (t, z, xp, yp))


# ---- B. stored lines ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain(lib):
    """The 68 lines of each of the 65 pairs from the step kernels of section A, chained in
    loop order: uint32 (65, 68, 72)."""
    prs = K.pairs()
    n = len(prs)
    pw = words([list(p) for p, _ in prs])                      # xp | yp
    qw = words([f2c(*q) for _, q in prs])                      # xq | yq
    one = words([[1, 0]])[0]
    t = np.concatenate([qw, np.tile(one, (n, 1))], axis=1)     # T = (xq, yq, 1)
    lines = np.zeros((n, K.N_LINES, LINE_WORDS), np.uint32)
    for j, kind in enumerate(K.loop_schedule()):
        a = np.concatenate([t, pw], axis=1)
        out = run1(lib, P_DBL, 0, a) if kind == "dbl" else run1(lib, P_ADD, 0, a, qw)
        t, lines[:, j, :] = out[:, :72], out[:, 72:]
    return lines


def soa(chain, n):
    """The layout of bls_pairing.h: word w of line j of pair q at (j * 72 + w) * n + q."""
    return np.ascontiguousarray(chain[:n].transpose(1, 2, 0)).reshape(-1)


@pytest.mark.parametrize("var", [L_LINES, L_LINES_QMEM], ids=["miller_lines", "miller_lines_qmem"])
@pytest.mark.parametrize("n", K.LINE_PAIR_COUNTS)
def test_stored_lines(lib, chain, n, var):
    """Every word of 68 x 72 x n_pairs written, at its SoA place, bit-identical to the chained
    step outputs; the guard on both sides untouched; line_get reads back what line_put wrote."""
    got, guard = run_lines(lib, var, K.pairs()[:n])
    assert np.all(guard == SENTINEL)
    want = soa(chain, n)
    assert got.shape == want.shape
    assert not np.any((got == SENTINEL) & (want != SENTINEL)), "a word was never written"
    assert np.array_equal(got, want)
    back = np.zeros(n * K.N_LINES * LINE_WORDS, np.uint32)
    assert lib.lbt_pairing_line_get(n, np.ascontiguousarray(got).ctypes.data, back.ctypes.data) == 0
    assert np.array_equal(back.reshape(n, K.N_LINES, LINE_WORDS), chain[:n])


def test_stored_lines_infinity(lib, chain):
    """miller_lines with P, Q or both flagged infinite (junk coordinates) stores 68 unit lines
    (l0 = 1, l1 = l4 = 0); the finite pair beside them is untouched by that branch."""
    prs = K.pairs()[:4]
    got, guard = run_lines(lib, L_LINES, prs, p_inf=(0, 2), q_inf=(1, 2))
    assert np.all(guard == SENTINEL)
    got = got.reshape(K.N_LINES, LINE_WORDS, 4)
    unit = words([[1, 0, 0, 0, 0, 0]])[0]
    for q in range(3):
        assert np.array_equal(got[:, :, q], np.tile(unit, (K.N_LINES, 1))), q
    assert np.array_equal(got[:, :, 3], chain[3])


# ---- C. Miller loop ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def lane_miller(lib):
    """One-lane miller_loop of the eight section C pairs and of pair 64: {pair: 144 words}."""
    idx = list(range(K.MAX_MILLER_PAIRS)) + [64]
    prs = [K.pairs()[i] for i in idx]
    out = run1(lib, P_MILLER, 0, words([list(p) for p, _ in prs]), words([f2c(*q) for _, q in prs]))
    return dict(zip(idx, out))


def f12_of(row):
    r = raw(row)
    assert all(v < P for v in r), "non-canonical limbs"
    return C.f12_unflat([C.unmont(x) for x in r])


@pytest.mark.parametrize("i", range(K.MAX_MILLER_PAIRS))
def test_miller_loop(lane_miller, i):
    """The device's f and the oracle's differ by an Fp2 factor and nothing else (the lines are
    scaled in Fp2), and the oracle's final exponentiation of the device's f is the pairing."""
    f = f12_of(lane_miller[i])
    assert K.fp2_factor_only(f, K.oracle_miller(i))
    assert O.final_exp(f) == K.oracle_pairing(i)


@pytest.mark.parametrize("n", [1, 65])
def test_wc_miller_from_lines(lib, chain, lane_miller, n):
    """Bit-identical to the one-lane miller_loop of the same pair (the same exact field
    computation, canonical outputs), at q = 0 and q = n_pairs - 1."""
    qs = np.array(sorted({0, n - 1}), np.uint32)
    lines = soa(chain, n)
    out = np.zeros((len(qs), 144), np.uint32)
    assert lib.lbt_wc_miller(n, lines.ctypes.data, len(qs), qs.ctypes.data, out.ctypes.data) == 0
    for q, row in zip(qs, out):
        assert np.array_equal(row, lane_miller[int(q)]), q


# ---- D. final exponentiation -------------------------------------------------------------
def f12_words(vals):
    return words([C.f12_flat(v) for v in vals])


@pytest.fixture(scope="module")
def lane_final(lib):
    return run1(lib, P_FINAL_EXP, 0, f12_words([f for _, f, _ in K.final_exp_inputs()]))


def test_final_exp(lane_final):
    """One-lane final_exp == the oracle's f^(3 (p^12 - 1) / r), exactly."""
    for (name, _, to_one), row, want in zip(K.final_exp_inputs(), lane_final, K.final_exp_expected()):
        assert raw(row) == mont_all(C.f12_flat(want)), name
        if to_one:
            assert O.f12_is_one(want), name


@pytest.mark.parametrize("var", [0, 1], ids=["dst_distinct", "in_place"])
def test_wc_final_exp(lib, lane_final, var):
    """Bit-identical to the one-lane result, also in place (k_tail's form); wc_is_one on each
    output is the oracle's f12_is_one."""
    out, flags = runw(lib, W_FINAL_EXP, 0, var, f12_words([f for _, f, _ in K.final_exp_inputs()]))
    assert np.array_equal(out, lane_final)
    assert [bool(x) for x in flags] == [O.f12_is_one(w) for w in K.final_exp_expected()]
    assert any(flags) and not all(flags)


def test_wc_is_one_rejects_near_one(lib):
    """False on 1 with a single 1 added at each of the other eleven positions and on zero;
    true on one."""
    vals = K.not_one_inputs() + [O.F12_ONE]
    _, flags = runw(lib, W_IS_ONE, 0, 0, f12_words(vals))
    assert [int(x) for x in flags] == [0] * (len(vals) - 1) + [1]


def test_final_exp_of_zero(lib):
    """f = 0 has no inverse, so the oracle defines nothing.  Both device forms return the zero
    element (fp12_inv's inversion maps 0 to 0, and every later step is a product with it):
    they agree and the result is not one, so a zero Miller product never verifies."""
    a = f12_words([C.f12_unflat([0] * 12)])
    lane = run1(lib, P_FINAL_EXP, 0, a)
    for var in (0, 1):
        out, flags = runw(lib, W_FINAL_EXP, 0, var, a)
        assert np.array_equal(out, lane) and int(flags[0]) == 0
    assert raw(lane[0]) != mont_all([1] + [0] * 11)


def test_exp_x(lib):
    """conj(a^|x|) on cyclotomic inputs and on 1: one-lane fp12_exp_x, wc_exp_x with
    dst != src and with dst == src (wc_final_exp's call)."""
    a = f12_words(K.exp_x_inputs())
    want = [mont_all(C.f12_flat(w)) for w in K.exp_x_expected()]
    assert [raw(r) for r in run1(lib, P_EXP_X, 0, a)] == want
    for var in (0, 1):
        assert [raw(r) for r in runw(lib, W_EXP_X, 0, var, a)[0]] == want, var


# ---- E. wc_apply -------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.PROGRAMS)
def test_wc_apply(lib, name):
    """Every program under every aliasing form the product uses, on the field edge cases, on
    random elements and on the extreme patterns of every operand form (p - 1 where the form's
    coefficient is positive and 0 where it is negative, and the opposite): the lazy sums of
    lz_sum at +w (p - 1) and at -w (p - 1).  Expected: the Python evaluation of the generated
    program modulo p and, where the program is an Fp12 operation on any input, the oracle."""
    cases = K.apply_cases(name)
    a = words([x for x, _ in cases])
    b = words([y for _, y in cases])
    wop = W.INDEX[name]
    first = None
    for var in K.FORMS[name]:
        got = [raw(r) for r in runw(lib, W_APPLY, wop, var, a, b)[0]]
        for (x, y), g in zip(cases, got):
            if var == 3:
                y = x
            elif name in K.FROBS and var != 4:
                y = K.gammas(K.FROBS[name])     # the device's own gamma slots (wc_init_gammas)
            assert g == mont_all(W.run_named(name, x, y)), (name, var, x, y)
            want = K.oracle_apply(name, x, y) if var != 4 else None
            if want is not None:
                assert g == mont_all(want), (name, var, x, y)
        if var in (0, 1):
            first = got if first is None else first
            assert got == first, (name, var)
    if name == "MUL":  # a == b must equal SQR
        sq = [raw(r) for r in runw(lib, W_APPLY, W.INDEX["SQR"], 0, a, a)[0]]
        assert [raw(r) for r in runw(lib, W_APPLY, wop, 3, a, b)[0]] == sq
    if name == "LINE":  # the result must not depend on slots 6..11 of the line operand
        other = words([K.with_line_junk(y, [7, P - 3, 1 << 379, 12345, P - 1, 2]) for _, y in cases])
        assert [raw(r) for r in runw(lib, W_APPLY, wop, 0, a, other)[0]] == first


def test_wc_slot_helpers(lib):
    """wc_load12 -> wc_store, through wc_copy, and wc_set_one: bit-exact round trips."""
    a = f12_words(C.f12_values(4, 4300))
    for var in (0, 1):
        out, _ = runw(lib, W_SLOTS, 0, var, a)
        assert np.array_equal(out, a), var
    out, _ = runw(lib, W_SLOTS, 0, 2, a[:2])
    assert [raw(r) for r in out] == [mont_all([1] + [0] * 11)] * 2


# ---- F. the product's pairing entry ------------------------------------------------------
def gt_bytes(f):
    return b"".join(c.to_bytes(48, "big") for c in C.f12_flat(f))


def test_device_pairing_infinity_and_multiples(device):
    """lb_pairing with an infinite P, an infinite Q and both returns one; e([a]P, [b]Q) for two
    (a, b) equals the oracle's value byte for byte."""
    prs = K.pairs()
    inf1, inf2 = O.g1_to_bytes(None, compressed=False), O.g2_to_bytes(None, compressed=False)
    g1 = [inf1, O.g1_to_bytes(O.G1, compressed=False), inf1]
    g2 = [O.g2_to_bytes(O.G2, compressed=False), inf2, inf2]
    for i in (2, 4):
        g1.append(O.g1_to_bytes(prs[i][0], compressed=False))
        g2.append(O.g2_to_bytes(prs[i][1], compressed=False))
    out = device.pairing(g1, g2)
    assert out[:3] == [gt_bytes(O.F12_ONE)] * 3
    assert out[3:] == [gt_bytes(K.oracle_pairing(2)), gt_bytes(K.oracle_pairing(4))]
