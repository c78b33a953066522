"""GPU checks of the one-lane group law (lodestar_amd/csrc/bls_curve.h) on G1 and G2,
at the branches no pipeline reaches: P + P and P + (-P) under equal and different Z,
infinity (Z = 0 with junk X, Y) on either side, the shared-Z GLV ladder behind every
r * pk and r * sig, the subgroup checks on points of the curve outside the subgroup
(a raw point, and Q + T with T in the cofactor torsion), and the ZCash encoders.

Points go in and come out as raw Montgomery limbs (Jacobian X | Y | Z) and are
normalised here (x = X / Z^2, y = Y / Z^3); every expected value is the pure-Python
oracle's.  The HIP side is tests/native/curve_selftest.hip (built by build(); test-only)."""
import ctypes
import os
import random

import numpy as np
import pytest

from oracle import bls12_381 as O
from tests import field_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (LB_CURVE_SELFTEST: another build of the same self-test)
LIB = os.environ.get("LB_CURVE_SELFTEST") or os.path.join(ROOT, "tests", "native", "libcurve_selftest.so")
P = O.P
LAMBDA = (-O.X_ABS * O.X_ABS) % O.R

pytestmark = pytest.mark.gpu

C_DBL, C_ADD, C_ADD_AFF, C_NEG, C_EQ, C_TO_AFF = range(6)
C_PAIR_TO_AFF = 10
C_MUL_U64, C_MUL_GLV, C_MUL_XABS = 20, 21, 22
C_PSI, C_GLV_ENDO, C_IN_SUBGROUP = 30, 31, 32
C_SERIALIZE, C_COMPRESS = 40, 41

GROUPS = [1, 2]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail("tests/native/libcurve_selftest.so missing: run __graft_entry__.build()")
    L = ctypes.CDLL(LIB)
    L.lbt_curve_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.lbt_curve_op_widths.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return L


# ---- per-group helpers ------------------------------------------------------------------
class Grp:
    def __init__(self, g):
        self.g = g
        self.F = O.FP if g == 1 else O.FP2
        self.E = O.E1 if g == 1 else O.E2
        self.gen = O.G1 if g == 1 else O.G2
        self.rng = random.Random(1000 + g)
        # subgroup points (small multiples are cheap for the oracle) and Z values
        self.pts = [self.E.mul(self.gen, k) for k in (1, 2, 3, 5, 0xFFFFFFFF, self.rng.getrandbits(64),
                                                       self.rng.getrandbits(64), self.rng.getrandbits(64))]
        self.zs = [self.F.one, self.rand_f(), self.rand_f(), self.F.neg(self.F.one)]

    def rand_f(self):
        return self.rng.randrange(1, P) if self.g == 1 else (self.rng.randrange(1, P), self.rng.randrange(1, P))

    def coeffs(self, v):
        return [C.mont(v)] if self.g == 1 else [C.mont(v[0]), C.mont(v[1])]

    def jac(self, pt, z=None):
        """Jacobian coefficients of pt under Z = z; pt None -> Z = 0 with junk X, Y."""
        F = self.F
        if pt is None:
            return self.coeffs(self.rand_f()) + self.coeffs(self.rand_f()) + self.coeffs(F.zero)
        z = F.one if z is None else z
        z2 = F.sqr(z)
        return self.coeffs(F.mul(pt[0], z2)) + self.coeffs(F.mul(pt[1], F.mul(z2, z))) + self.coeffs(z)

    def aff(self, pt):
        """(coefficients, inf flag); an infinite affine operand carries junk x, y."""
        if pt is None:
            return self.coeffs(self.rand_f()) + self.coeffs(self.rand_f()), 1
        return self.coeffs(pt[0]) + self.coeffs(pt[1]), 0

    def field(self, ws):
        v = [C.unmont(x) for x in C.ints(np.asarray(ws).reshape(self.g, 12))]
        return v[0] if self.g == 1 else (v[0], v[1])

    def norm(self, row):
        """X | Y | Z limbs -> affine oracle point (None = infinity)."""
        n = 12 * self.g
        X, Y, Z = (self.field(row[i * n:(i + 1) * n]) for i in range(3))
        if Z == self.F.zero:
            return None
        return self.E._to_affine(X, Y, Z)


@pytest.fixture(scope="module", params=GROUPS, ids=["g1", "g2"])
def grp(request):
    return Grp(request.param)


def words(rows_):
    """rows of Fp coefficients -> uint32 (n, 12 * len(row))."""
    return np.stack([C.limbs(r, 12).reshape(-1) for r in rows_])


def run(lib, op, g, var, a, b=None, k=None):
    w = (ctypes.c_uint32 * 3)()
    assert lib.lbt_curve_op_widths(op, g, w) == 0, (op, g)
    a = np.ascontiguousarray(a, np.uint32)
    n = a.shape[0]
    assert a.shape[1] == w[0], (a.shape, w[0])
    bp = kp = None
    if w[1]:
        b = np.ascontiguousarray(b, np.uint32)
        assert b.shape == (n, w[1]), (b.shape, w[1])
        bp = b.ctypes.data
    if k is not None:
        k = np.ascontiguousarray(np.array(k, np.uint64))
        assert k.shape == (n,)
        kp = k.ctypes.data
    out = np.zeros((n, w[2]), np.uint32)
    rc = lib.lbt_curve_op(op, g, var, n, a.ctypes.data, bp, kp, out.ctypes.data)
    assert rc == 0, rc
    return out


def aff_words(grp, pts):
    rows_, flags = zip(*(grp.aff(p) for p in pts))
    return np.concatenate([words(rows_), np.array(flags, np.uint32).reshape(-1, 1)], axis=1)


def add_cases(grp):
    """(P, Zp, Q, Zq): generic, P + P and P + (-P) under equal and different Z, infinity
    on either side and on both."""
    E, pts, zs = grp.E, grp.pts, grp.zs
    cases = []
    for i, p in enumerate(pts):
        q = pts[(i + 3) % len(pts)]
        cases.append((p, zs[i % 4], q, zs[(i + 1) % 4]))
        cases.append((p, zs[0], q, zs[0]))
        for zp, zq in ((zs[0], zs[0]), (zs[1], zs[1]), (zs[1], zs[2]), (zs[0], zs[2]), (zs[3], zs[0])):
            cases.append((p, zp, p, zq))             # doubling branch
            cases.append((p, zp, E.neg(p), zq))      # P + (-P)
        cases.append((None, None, q, zs[i % 4]))
        cases.append((p, zs[i % 4], None, None))
    cases.append((None, None, None, None))
    return cases


# ---- group law --------------------------------------------------------------------------
@pytest.mark.parametrize("var", [0, 1, 2])
def test_jac_add(lib, grp, var):
    cases = add_cases(grp)
    a = words([grp.jac(p, zp) for p, zp, _, _ in cases])
    b = words([grp.jac(q, zq) for _, _, q, zq in cases])
    out = run(lib, C_ADD, grp.g, var, a, b)
    for (p, _, q, _), row in zip(cases, out):
        assert grp.norm(row) == grp.E.add(p, q), (p, q)


def test_jac_add_same_object_and_dbl(lib, grp):
    """jac_add(r, p, p) with one object, jac_dbl out of place and in place (the ladders'
    jac_dbl(acc, acc)), doubling of infinity."""
    pts = [(p, z) for p in grp.pts for z in grp.zs[:3]] + [(None, None)] * 2
    a = words([grp.jac(p, z) for p, z in pts])
    want = [grp.E.add(p, p) for p, _ in pts]
    assert [grp.norm(r) for r in run(lib, C_ADD, grp.g, 3, a, a)] == want
    assert [grp.norm(r) for r in run(lib, C_DBL, grp.g, 0, a)] == want
    assert [grp.norm(r) for r in run(lib, C_DBL, grp.g, 1, a)] == want


@pytest.mark.parametrize("var", [0, 1])
def test_jac_add_aff(lib, grp, var):
    """Mixed addition: generic, Q = P (doubling branch, P under Z != 1 too), Q = -P,
    infinite P, an affine `inf` operand, both."""
    cases = [(p, zp, q) for p, zp, q, _ in add_cases(grp)]
    a = words([grp.jac(p, zp) for p, zp, _ in cases])
    out = run(lib, C_ADD_AFF, grp.g, var, a, aff_words(grp, [q for _, _, q in cases]))
    for (p, _, q), row in zip(cases, out):
        assert grp.norm(row) == grp.E.add(p, q), (p, q)


@pytest.mark.parametrize("var", [0, 1])
def test_jac_neg(lib, grp, var):
    pts = [(p, z) for p in grp.pts[:4] for z in grp.zs] + [(None, None)]
    out = run(lib, C_NEG, grp.g, var, words([grp.jac(p, z) for p, z in pts]))
    assert [grp.norm(r) for r in out] == [grp.E.neg(p) for p, _ in pts]


def test_jac_eq(lib, grp):
    """The same point under three different Z, a differing Y (P against -P), a differing
    X, infinity against infinity (different junk) and against a finite point."""
    E, zs = grp.E, grp.zs
    cases = []
    for i, p in enumerate(grp.pts):
        for z1 in zs[:3]:
            for z2 in zs[:3]:
                cases.append((p, z1, p, z2, True))
                cases.append((p, z1, E.neg(p), z2, False))
        cases.append((p, zs[1], grp.pts[(i + 1) % len(grp.pts)], zs[2], False))
        cases.append((p, zs[1], None, None, False))
        cases.append((None, None, p, zs[2], False))
    cases.append((None, None, None, None, True))
    a = words([grp.jac(p, zp) for p, zp, _, _, _ in cases])
    b = words([grp.jac(q, zq) for _, _, q, zq, _ in cases])
    assert [bool(r[0]) for r in run(lib, C_EQ, grp.g, 0, a, b)] == [c[4] for c in cases]
    assert all(r[0] == 1 for r in run(lib, C_EQ, grp.g, 3, a, b))  # jac_eq(p, p), infinity included


def test_jac_to_aff(lib, grp):
    pts = [(p, z) for p in grp.pts for z in grp.zs] + [(None, None)] * 2
    out = run(lib, C_TO_AFF, grp.g, 0, words([grp.jac(p, z) for p, z in pts]))
    n = 12 * grp.g
    for (p, _), row in zip(pts, out):
        assert bool(row[2 * n]) == (p is None)
        if p is not None:
            assert (grp.field(row[:n]), grp.field(row[n:2 * n])) == p


def test_jac_pair_to_aff(lib):
    """One shared inversion for a G1 and a G2 point.  With an infinite input only the
    `inf` flag on that side is compared; the finite side must still be exact."""
    g1, g2 = Grp(1), Grp(2)
    cases = []
    for i in range(8):
        p, q = g1.pts[i], g2.pts[(i + 2) % 8]
        cases.append((p, g1.zs[i % 4], q, g2.zs[(i + 1) % 4]))
        cases.append((None, None, q, g2.zs[i % 4]))
        cases.append((p, g1.zs[(i + 2) % 4], None, None))
    cases.append((None, None, None, None))
    a = words([g1.jac(p, zp) + g2.jac(q, zq) for p, zp, q, zq in cases])
    out = run(lib, C_PAIR_TO_AFF, 1, 0, a)
    for (p, _, q, _), row in zip(cases, out):
        assert bool(row[24]) == (p is None) and bool(row[25 + 48]) == (q is None)
        if p is not None:
            assert (g1.field(row[:12]), g1.field(row[12:24])) == p
        if q is not None:
            assert (g2.field(row[25:49]), g2.field(row[49:73])) == q


# ---- scalar ladders ---------------------------------------------------------------------
def ladder_bases(grp):
    return [(grp.pts[0], None), (grp.pts[5], None), (grp.pts[6], grp.zs[1]), (grp.pts[3], grp.zs[2]), (None, None)]


@pytest.mark.parametrize("var", [0, 1])
def test_jac_mul_u64(lib, grp, var):
    ks = [0, 1, 2, 1 << 63, (1 << 64) - 1, 3, grp.rng.getrandbits(64)]
    cases = [(p, z, k) for p, z in ladder_bases(grp) for k in ks]
    out = run(lib, C_MUL_U64, grp.g, var, words([grp.jac(p, z) for p, z, _ in cases]), k=[c[2] for c in cases])
    for (p, _, k), row in zip(cases, out):
        assert grp.norm(row) == grp.E.mul(p, k), hex(k)


@pytest.mark.parametrize("var", [0, 1])
def test_jac_mul_glv(lib, grp, var):
    """[a + b lambda]P with the product's constants (LB_G1_BETA/BETA2, LB_G2_OMEGA/OMEGA2):
    lambda = -x^2 mod r, a the low and b the high 32 bits of raw."""
    raws = [0, 1, 1 << 32, (1 << 32) + 1, 0xFFFFFFFF, 0xFFFFFFFF00000000, (1 << 64) - 1, 0x8000000000000001,
            2, 3 << 32, 0x0000000100000002, 0x0000000200000001]
    raws += [grp.rng.getrandbits(64) for _ in range(6)]
    cases = [(p, z, raw) for p, z in ladder_bases(grp) for raw in raws]
    out = run(lib, C_MUL_GLV, grp.g, var, words([grp.jac(p, z) for p, z, _ in cases]), k=[c[2] for c in cases])
    memo = {}
    for (p, _, raw), row in zip(cases, out):
        k = ((raw & 0xFFFFFFFF) + (raw >> 32) * LAMBDA) % O.R
        if (p, k) not in memo:
            memo[(p, k)] = grp.E.mul(p, k)
        assert grp.norm(row) == memo[(p, k)], hex(raw)


@pytest.mark.parametrize("var", [0, 1])
def test_jac_mul_xabs_and_endomorphisms(lib, grp, var):
    """[|x|]P, the GLV endomorphism (= [lambda]P on the subgroup) and, on G2, psi."""
    pts = [(p, z) for p, z in ladder_bases(grp)] + [(grp.pts[1], grp.zs[3]), (grp.pts[7], grp.zs[2])]
    a = words([grp.jac(p, z) for p, z in pts])
    assert [grp.norm(r) for r in run(lib, C_MUL_XABS, grp.g, var, a)] == [grp.E.mul(p, O.X_ABS) for p, _ in pts]
    assert [grp.norm(r) for r in run(lib, C_GLV_ENDO, grp.g, var, a)] == [grp.E.mul(p, LAMBDA) for p, _ in pts]
    if grp.g == 2:
        assert [grp.norm(r) for r in run(lib, C_PSI, 2, var, a)] == [O.psi(p) for p, _ in pts]


# ---- subgroup checks --------------------------------------------------------------------
def raw_point(grp):
    """An on-curve point with small x, outside the subgroup."""
    F, E = grp.F, grp.E
    x = 3
    while True:
        x += 1
        xf = x if grp.g == 1 else (x, 0)
        rhs = F.add(F.mul(F.sqr(xf), xf), E.b)
        y = O.fp_sqrt(rhs) if grp.g == 1 else (O.f2_sqrt(rhs) if O.f2_is_square(rhs) else None)
        if y is not None:
            pt = (xf, y)
            assert E.on_curve(pt)
            if E.mul(pt, O.R) is not None:
                return pt


def test_in_subgroup(lib, grp):
    """Members: the generator, multiples, infinity.  Non-members: a raw curve point, and
    Q + T with Q in the subgroup and T = [r] * (raw point) in the cofactor torsion -- the
    shape the pairing equation alone does not reject."""
    E = grp.E
    raw = raw_point(grp)
    if grp.g == 1:
        assert raw[0] == 4
    T = E.mul(raw, O.R)
    assert T is not None and E.on_curve(T)
    cases = [(p, z, True) for p in grp.pts for z in grp.zs[:2]] + [(None, None, True)]
    for z in grp.zs[:3]:
        cases.append((raw, z, False))
        cases.append((T, z, False))
        cases.append((E.add(grp.pts[0], T), z, False))
        cases.append((E.add(grp.pts[6], E.neg(T)), z, False))
    out = run(lib, C_IN_SUBGROUP, grp.g, 0, words([grp.jac(p, z) for p, z, _ in cases]))
    assert [bool(r[0]) for r in out] == [c[2] for c in cases]


# ---- ZCash encoders ---------------------------------------------------------------------
def test_serialize_compress(lib, grp):
    """Against O.g1_to_bytes / O.g2_to_bytes in both forms: subgroup points and their
    negatives, infinity, and y on either side of (p - 1) / 2.  The encoders never evaluate
    the curve equation, so the threshold cases are synthetic (x, y) pairs: a curve point
    with y = (p +- 1) / 2, or a G2 point with y.c1 = 0, needs a cube root in the field,
    which the oracle does not offer, and none was searched for."""
    H = C.HALF
    pts = list(grp.pts) + [grp.E.neg(p) for p in grp.pts] + [None]
    x = grp.pts[2][0]
    if grp.g == 1:
        pts += [(x, y) for y in (H, H + 1, H - 1, 0, 1, P - 1)] + [(0, 1), (P - 1, H)]
    else:
        pts += [(x, (y0, y1)) for y1 in (0, H, H + 1, 1, P - 1) for y0 in (0, H, H + 1, 1, P - 1)]
        pts += [((0, P - 1), (H + 1, 0)), ((P - 1, 0), (H, 0))]
    to_bytes = O.g1_to_bytes if grp.g == 1 else O.g2_to_bytes
    a = aff_words(grp, pts)
    got = [bytes(r.view(np.uint8)) for r in run(lib, C_SERIALIZE, grp.g, 0, a)]
    assert got == [to_bytes(p, compressed=False) for p in pts]
    got = [bytes(r.view(np.uint8)) for r in run(lib, C_COMPRESS, grp.g, 0, a)]
    assert got == [to_bytes(p, compressed=True) for p in pts]
