"""Inputs and oracle expectations shared by tests/test_gpu_pairing.py (GPU) and
tests/test_pairing_cases.py (CPU: the case lists really hold what they claim).

Sections follow the GPU file: A Miller steps, B stored lines, C Miller loop, D final
exponentiation, E wc_apply.  All values here are canonical integers / oracle tuples;
the GPU test converts to Montgomery limbs."""
import functools
import random

from oracle import bls12_381 as O
from tests import field_cases as C
from tests import wc12_helper as W

P = O.P

# caps (per-test cost: one wave per case; the Python final exponentiation is the slow part)
MAX_FINAL_EXP_INPUTS = 24
MAX_MILLER_PAIRS = 8
LINE_PAIR_COUNTS = (1, 3, 64, 65)
N_LINES = 68


# ---- A. Miller steps ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def e2_points():
    """E2 points of the oracle: generator multiples (small and 64-bit) and a hash output."""
    rng = random.Random(4001)
    pts = [O.E2.mul(O.G2, k) for k in (1, 2, 3, rng.getrandbits(64))]
    pts.append(O.hash_to_g2(b"pairing_cases step"))
    return pts


@functools.lru_cache(maxsize=None)
def step_scales():
    """Z of the homogeneous projective T: 1, -1 and two random Fp2 values."""
    rng = random.Random(4002)
    return [(1, 0), (P - 1, 0)] + [(rng.randrange(1, P), rng.randrange(1, P)) for _ in range(2)]


@functools.lru_cache(maxsize=None)
def step_p_coords():
    return [0, 1, P - 1, random.Random(4003).randrange(2, P - 1)]


@functools.lru_cache(maxsize=None)
def step_cases():
    """(T affine, Z, Q affine, xp, yp): every point under every scale with every (xp, yp) of
    {0, 1, p - 1, random}^2; Q (the addition step's affine operand) is the next point of the
    list, so Q != +-T.  P = (xp, yp) need not be on the curve: the lines are polynomial in it."""
    pts, xs = e2_points(), step_p_coords()
    return [(t, z, pts[(i + 1) % len(pts)], xp, yp)
            for i, t in enumerate(pts) for z in step_scales() for xp in xs for yp in xs]


def proj(pt, z):
    """(X, Y, Z) with x = X / Z, y = Y / Z."""
    return (O.f2_mul(pt[0], z), O.f2_mul(pt[1], z), z)


def unproj(X, Y, Z):
    zi = O.f2_inv(Z)
    return (O.f2_mul(X, zi), O.f2_mul(Y, zi))


def oracle_line(lam, t, p):
    """(c0, c1, c4) of the oracle's line through t with slope lam, evaluated at p."""
    l = O._line(lam, t[0], t[1], p)
    return (l[0][0], l[0][1], l[1][1])


def tangent_slope(t):
    return O.f2_mul(O.f2_mul_fp(O.f2_sqr(t[0]), 3), O.f2_inv(O.f2_add(t[1], t[1])))


def chord_slope(t, q):
    return O.f2_mul(O.f2_sub(q[1], t[1]), O.f2_inv(O.f2_sub(q[0], t[0])))


def proportional(l, c):
    """(l0 : l1 : l4) == (c0 : c1 : c4) as projective triples over Fp2: every pair by
    cross-multiplication, and l not all zero (c never is: c0 or c4 would have to vanish
    together with the slope)."""
    if all(O.f2_is_zero(x) for x in l) or all(O.f2_is_zero(x) for x in c):
        return False
    return all(O.f2_mul(l[i], c[j]) == O.f2_mul(l[j], c[i]) for i in range(3) for j in range(i + 1, 3))


# ---- B / C. pairs ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pairs():
    """65 different (P, Q), P in G1 and Q in G2, affine.  The first MAX_MILLER_PAIRS are the
    Miller-loop cases of section C: the generators, -G1, small and 64-bit multiples, two
    hash_to_g2 outputs."""
    rng = random.Random(4004)
    k64 = [rng.getrandbits(64) | 1 << 63 for _ in range(5)]
    g1, g2 = O.G1, O.G2
    out = [(g1, g2),
           (O.E1.neg(g1), g2),
           (O.E1.mul(g1, 2), O.E2.mul(g2, 3)),
           (O.E1.mul(g1, 5), O.E2.neg(O.E2.mul(g2, 7))),
           (O.E1.mul(g1, k64[0]), O.E2.mul(g2, k64[1])),
           (O.E1.mul(g1, k64[2]), O.E2.mul(g2, k64[3])),
           (O.E1.mul(g1, 3), O.hash_to_g2(b"pairing_cases miller 0")),
           (O.E1.mul(g1, k64[4]), O.hash_to_g2(b"pairing_cases miller 1"))]
    p, q = O.E1.mul(g1, 100), O.E2.mul(g2, 200)
    while len(out) < max(LINE_PAIR_COUNTS):
        out.append((p, q))
        p, q = O.E1.add(p, g1), O.E2.add(q, O.E2.double(g2))
    return out


@functools.lru_cache(maxsize=None)
def oracle_miller(i):
    return O.miller_loop(*pairs()[i])


@functools.lru_cache(maxsize=None)
def oracle_pairing(i):
    return O.final_exp(oracle_miller(i))


def loop_schedule():
    """The step kinds of one Miller loop in order: 63 doublings, an addition after each set
    bit of |x| below the top one."""
    out = []
    for i in range(62, -1, -1):
        out.append("dbl")
        if (O.X_ABS >> i) & 1:
            out.append("add")
    return out


def fp2_factor_only(f, g):
    """f / g lies in Fp2 and is not zero: the two differ by an Fp2 factor and nothing else."""
    c = C.f12_flat(O.f12_mul(f, O.f12_inv(g)))
    return (c[0] or c[1]) and not any(c[2:])


# ---- D. final exponentiation -------------------------------------------------------------
def _embed(coeffs):
    return C.f12_unflat(list(coeffs) + [0] * (12 - len(coeffs)))


@functools.lru_cache(maxsize=None)
def final_exp_inputs():
    """(name, Fp12, must map to one).  1 and -1 are the list's Fp elements (the cap of 24
    inputs, MAX_FINAL_EXP_INPUTS, leaves no room for a random third); the Fp2 and Fp6 elements
    are random.  Flagged are the elements of a proper subfield and the Miller product."""
    rng = random.Random(4005)
    rnd = lambda n: [rng.randrange(1, P) for _ in range(n)]  # noqa: E731
    cases = [("one", O.F12_ONE, True), ("minus_one", _embed([P - 1]), True),
             ("fp2", _embed(rnd(2)), True), ("fp6", _embed(rnd(6)), True)]
    for pos in range(1, 12):
        c = [0] * 12
        c[pos] = 1
        cases.append(("unit_%d" % pos, C.f12_unflat(c), pos < 6))
    cases.append(("all_p_minus_1", C.f12_unflat([P - 1] * 12), False))
    cases += [("random_%d" % i, C.f12_unflat(rnd(12)), False) for i in range(4)]
    cases += [("miller_0", oracle_miller(0), False), ("miller_4", oracle_miller(4), False)]
    # pairs 0 and 1 are (G1, G2) and (-G1, G2)
    cases.append(("miller_product", O.f12_mul(oracle_miller(0), oracle_miller(1)), True))
    cases.append(("gt", oracle_pairing(2), False))
    return cases


@functools.lru_cache(maxsize=None)
def final_exp_expected():
    return [O.final_exp(f) for _, f, _ in final_exp_inputs()]


@functools.lru_cache(maxsize=None)
def not_one_inputs():
    """1 with a single 1 added at each of the other eleven positions, and zero."""
    out = []
    for pos in range(1, 12):
        c = [1] + [0] * 11
        c[pos] = 1
        out.append(C.f12_unflat(c))
    out.append(C.f12_unflat([0] * 12))
    return out


@functools.lru_cache(maxsize=None)
def exp_x_inputs():
    """Eight elements made cyclotomic by the easy part, and 1."""
    rng = random.Random(4006)
    src = [C.f12_unflat([rng.randrange(P) for _ in range(12)]) for _ in range(6)]
    src += [C.f12_unflat([P - 1] * 12), oracle_miller(0)]
    return [C.f12_cyclotomic(a) for a in src] + [O.F12_ONE]


@functools.lru_cache(maxsize=None)
def exp_x_expected():
    return [O.f12_conj(O.f12_pow(a, O.X_ABS)) for a in exp_x_inputs()]


# ---- E. wc_apply -------------------------------------------------------------------------
PROGRAMS = tuple(W.NAMES)
FROBS = {"FROB1": 1, "FROB2": 2, "FROB3": 3}
UNARY = ("SQR", "CYC", "CONJ")
# aliasing forms (the var argument of the self-test): 0 dst distinct, 1 dst == a, 2 dst == b,
# 3 b is a, 4 a Frobenius program with b from the host instead of the gamma slot
FORMS = {"MUL": (0, 1, 2, 3), "SQR": (0, 1), "CYC": (0, 1), "LINE": (0, 1), "FROB1": (0, 1, 4), "FROB2": (0, 1, 4),
         "FROB3": (0, 1, 4), "CONJ": (0, 1)}


@functools.lru_cache(maxsize=None)
def gammas(k):
    """B of LB_WC_FROBk: xi^(e (p^k - 1) / 6) at B[2e], B[2e + 1]; B[0], B[1] are not read."""
    g = [c for e in range(6) for c in O.f2_pow((1, 1), e * (P ** k - 1) // 6)]
    g[0] = g[1] = 0
    return g


def form_weights(form):
    pos = sum(c for c in form.d.values() if c > 0)
    neg = -sum(c for c in form.d.values() if c < 0)
    return pos, neg


def form_value(form, A, B):
    """The signed sum lz_sum forms before it adds kneg * p."""
    return sum(c * (A if kind == "A" else B)[i] for (kind, i), c in form.d.items())


def form_pattern(form, sign):
    """12 coefficients: p - 1 where sign * (the form's coefficient) > 0, else 0."""
    v = [0] * 12
    for (_, i), c in form.d.items():
        if c * sign > 0:
            v[i] = P - 1
    return v


LINE_JUNK = [P - 1, 1, (1 << 380) - 1, 0xFFFFFFFF, P - 2, 1 << 380]


def with_line_junk(b, junk=LINE_JUNK):
    """Slots 6..11 of the line operand hold whatever the product's LDS held: non-zero junk."""
    return list(b[:6]) + list(junk)


@functools.lru_cache(maxsize=None)
def extreme_cases(name):
    """For every operand form x_k, y_k of the program: the input that drives its signed sum to
    +(positive weight)(p - 1) and the one that drives it to -(negative weight)(p - 1), crossed
    with the same two patterns on the other operand.  Deduplicated (A, B) coefficient lists; a
    square program's B is its A."""
    prog, _ = W.program(name)
    seen, out = set(), []

    def push(a, b):
        if name == "LINE":
            b = with_line_junk(b)
        key = (tuple(a), tuple(b))
        if key not in seen:
            seen.add(key)
            out.append((list(a), list(b)))

    for x, y in prog.prods:
        if prog.square:
            for f in (x, y):
                for s in (1, -1):
                    a = form_pattern(f, s)
                    push(a, a)
        else:
            for sx in (1, -1):
                for sy in (1, -1):
                    push(form_pattern(x, sx), form_pattern(y, sy))
    return out


@functools.lru_cache(maxsize=None)
def edge_cases(name):
    """The Fp12 case set of tests/field_cases.py (0, 1, single coefficients, all p - 1, random)
    on both operands, and random elements."""
    rng = random.Random(4100 + W.INDEX[name])
    vals = [C.f12_flat(v) for v in C.f12_values(6, 4200)]
    n = len(vals)
    out = [(vals[i], vals[(5 * i + 1) % n]) for i in range(n)]
    out += [(vals[2], vals[2]), (vals[0], vals[0]), (vals[1], vals[2]), (vals[2], vals[1])]
    out += [([rng.randrange(P) for _ in range(12)], [rng.randrange(P) for _ in range(12)]) for _ in range(16)]
    if name == "CYC":  # cyclotomic inputs, where the program is a squaring
        out += [(C.f12_flat(a), C.f12_flat(a)) for a in exp_x_inputs()[:3]]
    if name == "LINE":
        out = [(a, with_line_junk(b)) for a, b in out]
    if name in UNARY:
        out = [(a, a) for a, _ in out]
    return out


def apply_cases(name):
    return edge_cases(name) + extreme_cases(name)


def oracle_apply(name, A, B):
    """The oracle's result where the program is an Fp12 operation on any input (None for
    LB_WC_CYC off the cyclotomic subgroup).  B of a Frobenius program must be gammas(k)."""
    a = C.f12_unflat(A)
    if name == "MUL":
        r = O.f12_mul(a, C.f12_unflat(B))
    elif name == "SQR":
        r = O.f12_sqr(a)
    elif name == "LINE":
        r = O.f12_mul(a, C.embed_line((B[0], B[1]), (B[2], B[3]), (B[4], B[5])))
    elif name in FROBS:
        r = C.f12_frob(a, FROBS[name])
    elif name == "CONJ":
        r = O.f12_conj(a)
    else:
        return None
    return C.f12_flat(r)
