"""Blob KZG commitments and proofs, CPU side: the restatement in tests/kzg_commit_helper.py
against tests/kzg_helper.py's evaluation (a commitment is f(tau), a proof the quotient at tau),
the MSM's digits, the G1 half of the trusted-setup parser, GpuKzg's throw side against a stub
device, and the C ABI's argument checks that need no GPU."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

from lodestar_amd import kzg, native
from tests import kzg_commit_helper as C
from tests import kzg_helper as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, N = K.R, K.N
TAU = K.TestSetup().tau


@pytest.fixture(scope="module")
def lag():
    return C.lagrange_scalars(TAU)


def dot(a, b):
    return sum(x * y for x, y in zip(a, b)) % R


def test_lagrange_scalars_evaluate_at_tau(lag):
    f = K.random_poly(11)
    assert dot(f, lag) == K.evaluate(f, TAU)
    assert sum(lag) % R == 1


@pytest.mark.parametrize("z", [2, 0x5EED % R * 0xABCDEF0123456789 % R, K.ROOTS[0], K.ROOTS[1], K.ROOTS[N - 1]])
def test_quotient_at_tau_is_the_proof_scalar(lag, z):
    f = K.random_poly(12)
    q, y = C.quotient(f, z)
    assert y == K.evaluate(f, z)
    if z in K.ROOTS:
        assert y == f[K.ROOTS.index(z)]
    assert dot(q, lag) == (K.evaluate(f, TAU) - y) * pow(TAU - z, -1, R) % R


def test_recode_round_trips_within_bounds():
    rng = random.Random(13)
    vals = [0, 1, 127, 128, 129, 255, 256, R - 1, R - 2, int.from_bytes(b"\x80" * 32, "big") % R,
            int.from_bytes(b"\x01" + b"\x81" * 31, "big")] + [128 * 256 ** j for j in range(31)] + \
           [129 * 256 ** j for j in range(31)] + [rng.randrange(R) for _ in range(2000)]
    top = 0
    for v in vals:
        assert v < R
        d = C.recode(v)
        assert len(d) == 32 and all(-127 <= x <= 128 for x in d)
        assert sum(x * 256 ** j for j, x in enumerate(d)) == v
        top = max(top, max(abs(x) for x in d))
    assert top == 128
    assert C.recode(128) == [128] + [0] * 31 and C.recode(129) == [-127, 1] + [0] * 30
    assert C.recode(int.from_bytes(b"\x01" + b"\x81" * 31, "big")) == [-127] + [-126] * 30 + [2]


def test_file_order_is_the_inverse_permutation():
    xs = list(range(N))
    fo = C.file_order(xs)
    assert [fo[K.brp(i)] for i in range(N)] == xs and fo[1] == N // 2


def test_trusted_setup_parser_takes_the_g1_lines():
    g1 = ["%096x" % (i + 1) for i in range(4096)]
    g2 = ["%0192x" % (1000 + i) for i in range(65)]
    text = "4096\n65\n" + "\n".join(g1 + g2) + "\n"
    out = kzg.parse_trusted_setup_g1(text)
    assert len(out) == 196608 and out == b"".join(bytes.fromhex(x) for x in g1)
    assert kzg.parse_trusted_setup(text) == bytes.fromhex(g2[1])
    with pytest.raises(kzg.KzgError):
        kzg.parse_trusted_setup_g1("4096\n65\n" + "\n".join(g1[:-1] + ["zz" * 48] + g2))
    with pytest.raises(kzg.KzgError):
        kzg.parse_trusted_setup_g1("4096\n65\n" + "\n".join(g1[:-1] + ["00" * 47] + g2))
    with pytest.raises(kzg.KzgError):
        kzg.parse_trusted_setup_g1("4096\n65\n" + "\n".join(g1 + g2[:64]))


class StubDevice:
    """Has the new methods; answers with recognisable bytes and the statuses it is told to."""

    def __init__(self):
        self.g1 = self.g2 = None
        self.status = {}
        self.calls = []

    def kzg_load_setup(self, tau):
        self.g2 = tau

    def kzg_load_setup_g1(self, g1):
        self.g1 = g1

    def _st(self, n):
        return [self.status.get(i, 0) for i in range(n)]

    def kzg_blob_commitments(self, blobs):
        self.calls.append(("commit", len(blobs)))
        return [bytes([0xC1]) * 48 for _ in blobs], self._st(len(blobs))

    def kzg_blob_proofs(self, blobs, commitments):
        self.calls.append(("prove", len(blobs)))
        return [bytes([0xC2]) * 48 for _ in blobs], self._st(len(blobs))

    def kzg_compute_proofs(self, blobs, zs):
        self.calls.append(("point", len(blobs)))
        return [bytes([0xC3]) * 48 for _ in blobs], [bytes([7]) * 32 for _ in blobs], self._st(len(blobs))


def test_gpu_kzg_commit_and_prove_against_a_stub_device(tmp_path):
    g1 = ["%096x" % (i + 1) for i in range(4096)]
    g2 = ["%0192x" % (1000 + i) for i in range(65)]
    path = tmp_path / "trusted_setup.txt"
    path.write_text("4096\n65\n" + "\n".join(g1 + g2) + "\n")
    dev = StubDevice()
    g = kzg.GpuKzg(dev)
    blob = bytes(K.BYTES_PER_BLOB)
    with pytest.raises(kzg.KzgError, match="not loaded"):
        g.blob_to_kzg_commitment(blob)
    order = []
    dev.kzg_load_setup_g1 = lambda g1, keep=dev.kzg_load_setup_g1: (order.append("g1"), keep(g1))
    dev.kzg_load_setup = lambda tau, keep=dev.kzg_load_setup: (order.append("g2"), keep(tau))
    g.load_trusted_setup(str(path))
    assert order == ["g1", "g2"]  # a refused G1 point must leave [tau]_2 as it was
    assert dev.g2 == bytes.fromhex(g2[1]) and dev.g1 == b"".join(bytes.fromhex(x) for x in g1)
    assert g.blob_to_kzg_commitment(blob) == bytes([0xC1]) * 48
    assert g.compute_blob_kzg_proof(blob, K.G1_INF) == bytes([0xC2]) * 48
    assert g.compute_kzg_proof(blob, bytes(32)) == (bytes([0xC3]) * 48, bytes([7]) * 32)
    assert g.blobs_to_kzg_commitments([]) == [] and g.compute_blob_kzg_proofs([], []) == []
    # more than one device call's worth is split, and item numbers count through the parts
    dev.calls.clear()
    n = native.LB_KZG_MAX_BLOBS + 2
    assert len(g.blobs_to_kzg_commitments([blob] * n)) == n
    assert dev.calls == [("commit", native.LB_KZG_MAX_BLOBS), ("commit", 2)]
    # lengths raise before the device is reached
    dev.calls.clear()
    for fn, args in ((g.blob_to_kzg_commitment, (blob[:-1],)), (g.compute_blob_kzg_proof, (blob[:-1], K.G1_INF)),
                     (g.compute_blob_kzg_proof, (blob, K.G1_INF[:-1])), (g.compute_kzg_proof, (blob, bytes(31))),
                     (g.compute_kzg_proof, (blob + b"\0", bytes(32))),
                     (g.compute_blob_kzg_proofs, ([blob, blob], [K.G1_INF]))):
        with pytest.raises(kzg.KzgError):
            fn(*args)
    assert dev.calls == []
    # a status raises, naming the item
    dev.status = {1: native.LB_KZG_BAD_BLOB}
    with pytest.raises(kzg.KzgError, match="item 1: BAD_BLOB"):
        g.blobs_to_kzg_commitments([blob, blob])
    dev.status = {0: native.LB_KZG_BAD_COMMITMENT}
    with pytest.raises(kzg.KzgError, match="item 0: BAD_COMMITMENT"):
        g.compute_blob_kzg_proof(blob, K.G1_INF)
    dev.status = {0: native.LB_KZG_BAD_SCALAR}
    with pytest.raises(kzg.KzgError, match="item 0: BAD_SCALAR"):
        g.compute_kzg_proof(blob, bytes(32))


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_kzg_commit_against_a_stub_backend():
    r = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "kzg_commit_host.js")],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "kzg commit host ok" in r.stdout, r.stdout + r.stderr


def test_c_abi_refuses_a_null_context():
    lib = native.load_library()
    buf = (ctypes.c_uint8 * 96)()
    bad = ctypes.c_int32(7)
    assert lib.lb_kzg_load_setup_g1(None, buf, ctypes.byref(bad)) == native.LB_ERR_INVALID_ARGUMENT
    assert lib.lb_kzg_setup_g1_loaded(None) == native.LB_ERR_INVALID_ARGUMENT
    assert lib.lb_kzg_blob_commitments(None, 0, None, None, None) == native.LB_ERR_INVALID_ARGUMENT
    assert lib.lb_kzg_blob_proofs(None, 0, None, None, None, None) == native.LB_ERR_INVALID_ARGUMENT
    assert lib.lb_kzg_compute_proofs(None, 0, None, None, None, None, None) == native.LB_ERR_INVALID_ARGUMENT
    assert lib.lb_kzg_g1_lincomb(None, 0, None, None, None) == native.LB_ERR_INVALID_ARGUMENT
    assert bad.value == 7
