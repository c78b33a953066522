"""Blob KZG verification, CPU side: the Python restatement (tests/kzg_helper.py) against the
mainnet KAT in tests/golden/kzg_mainnet_kat.json, the trusted-setup parser of
lodestar_amd/kzg.py, and the C ABI's argument checks that need no GPU."""
import ctypes
import json
import os
import shutil
import subprocess

import pytest

from lodestar_amd import kzg, native
from oracle import bls12_381 as O
from tests import kzg_helper as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(ROOT, "tests", "golden", "kzg_mainnet_kat.json")) as f:
        return json.load(f)


def test_helper_verifies_mainnet_kat_and_rejects_a_changed_y(kat):
    tau_g2 = O.g2_from_bytes(bytes.fromhex(kat["g2_tau"]))
    assert O.g2_in_subgroup(tau_g2)
    c, p = bytes.fromhex(kat["commitment"]), bytes.fromhex(kat["proof"])
    blob = K.blob_from_ints(K.kat_poly())
    z = K.compute_challenge(blob, c)
    y = K.evaluate(K.kat_poly(), z)
    assert K.fe(z).hex() == kat["z"] and K.fe(y).hex() == kat["y"]
    assert K.verify_kzg_proof_batch([c], [z], [y], [p], tau_g2) is True
    yb = bytearray(K.fe(y))
    yb[31] ^= 1
    assert K.verify_kzg_proof_batch([c], [z], [K.bytes_to_bls_field(bytes(yb))], [p], tau_g2) is False


def test_roots_of_unity():
    assert K.ROOTS[0] == 1 and K.ROOTS[1] == K.R - 1
    assert len(set(K.ROOTS)) == K.N
    assert all(pow(w, K.N, K.R) == 1 for w in K.ROOTS[:8])


def test_helper_test_setup_is_consistent():
    s = K.TestSetup()
    f = K.random_poly(7)
    blob, c, p, z, y = s.blob_case(f)
    assert K.verify_blob_kzg_proof_batch([blob], [c], [p], s.tau_g2_point) is True
    assert K.verify_kzg_proof_batch([c], [z], [(y + 1) % K.R], [p], s.tau_g2_point) is False


def test_trusted_setup_parser_takes_g2_line_1(tmp_path):
    g1 = ["%096x" % (i + 1) for i in range(4096)]
    g2 = ["%0192x" % (1000 + i) for i in range(65)]
    text = "4096\n65\n" + "\n".join(g1) + "\n" + "\n".join(g2) + "\n"
    assert kzg.parse_trusted_setup(text) == bytes.fromhex(g2[1])
    with pytest.raises(kzg.KzgError):
        kzg.parse_trusted_setup("4096\n64\n" + "\n".join(g1 + g2[:64]))
    with pytest.raises(kzg.KzgError):
        kzg.parse_trusted_setup("4096\n65\n" + "\n".join(g1 + g2[:64]))

    class FakeDevice:
        loaded = None

        def kzg_load_setup(self, tau):
            self.loaded = tau

    path = tmp_path / "trusted_setup.txt"
    path.write_text(text)
    dev = FakeDevice()
    g = kzg.GpuKzg(dev)
    g.load_trusted_setup(str(path))
    assert dev.loaded == bytes.fromhex(g2[1])
    with pytest.raises(kzg.KzgError, match="^Error trusted setup is already loaded$"):
        g.load_trusted_setup(str(path))
    g.free_trusted_setup()
    g.load_trusted_setup(str(path))
    for fn, args in ((g.blob_to_kzg_commitment, (b"",)), (g.compute_blob_kzg_proof, (b"", b""))):
        with pytest.raises(NotImplementedError, match="not implemented: use c-kzg"):
            fn(*args)


def test_gpu_kzg_raises_on_lengths_before_the_device():
    class NoDevice:
        def kzg_load_setup(self, tau):
            pass

        def kzg_verify_blob_proof_batch(self, *a):
            raise AssertionError("reached the device")

    g = kzg.GpuKzg(NoDevice())
    g._loaded = True
    blob = bytes(K.BYTES_PER_BLOB)
    with pytest.raises(kzg.KzgError):
        g.verify_blob_kzg_proof_batch([blob], [K.G1_INF, K.G1_INF], [K.G1_INF])
    with pytest.raises(kzg.KzgError):
        g.verify_blob_kzg_proof(blob[:-1], K.G1_INF, K.G1_INF)
    with pytest.raises(kzg.KzgError):
        g.verify_blob_kzg_proof(blob, K.G1_INF[:-1], K.G1_INF)
    g._loaded = False
    with pytest.raises(kzg.KzgError):
        g.verify_blob_kzg_proof(blob, K.G1_INF, K.G1_INF)


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_kzg_object_against_a_stub_backend():
    r = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "kzg_host.js")], capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "kzg host ok" in r.stdout, r.stdout + r.stderr


def test_c_abi_refuses_a_null_context():
    lib = native.load_library()
    ok = ctypes.c_int32(7)
    buf = (ctypes.c_uint8 * 96)()
    assert lib.lb_kzg_verify_blob_proof_batch(None, 0, None, None, None, ctypes.byref(ok), None,
                                              None) == native.LB_ERR_INVALID_ARGUMENT
    assert lib.lb_kzg_verify_proof_batch(None, 0, None, None, None, None, ctypes.byref(ok), None,
                                         None) == native.LB_ERR_INVALID_ARGUMENT
    assert lib.lb_kzg_load_setup(None, buf) == native.LB_ERR_INVALID_ARGUMENT
    assert lib.lb_kzg_setup_loaded(None) == native.LB_ERR_INVALID_ARGUMENT
    assert lib.lb_kzg_blob_challenges(None, 0, None, None, None, None, None) == native.LB_ERR_INVALID_ARGUMENT
    assert lib.lb_kzg_evaluate(None, 0, None, None, None, None) == native.LB_ERR_INVALID_ARGUMENT
    assert ok.value == 7
