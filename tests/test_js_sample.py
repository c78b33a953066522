"""syncBalances / computeProposers / syncCommittee on the JS host (tests/js/test_sample.js, a mock
backend under node), the addon's exports, and one run through the real addon on the GPU
(tests/js/gpu_sample.js) against the hashlib restatement of tests/sample_helper.py."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "lodestar_amd", "napi", "lodestar_bls.node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


def test_js_sample_hosts():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_sample.js")], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "0 failed" in r.stdout, r.stdout + r.stderr


def test_addon_exports_the_sample_calls():
    if not os.path.exists(ADDON):
        from lodestar_amd.napi import build as nb
        if not nb.available():
            pytest.skip("node headers not available")
        nb.build()
    script = ("const a = require(%r); const p = a.Context.prototype;"
              "if (typeof p.balanceTablePut !== 'function' || typeof p.sampleByBalance !== 'function') process.exit(3);"
              "console.log('sample calls ok');" % ADDON)
    r = subprocess.run([NODE, "-e", script], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert r.returncode == 0 and "sample calls ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_addon_sample_on_the_gpu(tmp_path):
    """Proposers and a sync committee through the real addon: keys, the expected indices and a
    signature of the whole committee come from here."""
    import hashlib
    import json
    import sys

    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sample_helper as SA
    from lodestar_amd.native import Device
    from oracle import bls12_381 as O
    n, size = 40, 24
    rnd = np.random.default_rng(11)
    active = rnd.permutation(n)[:30].astype(np.uint32)
    inc = rnd.integers(0, 33, n).astype(np.uint8)
    epoch_seed, seed = hashlib.sha256(b"js-proposers").digest(), hashlib.sha256(b"js-sync").digest()
    proposers = [SA.sample_rounds(s, active, inc, 32, 1, len(active))[0][0] for s in SA.slot_seeds(epoch_seed, 96)]
    committee, found, _ = SA.sample_rounds(seed, active, inc, 32, size, 1 << 22)
    assert found == size
    msg = hashlib.sha256(b"js-sync-msg").digest()
    dev = Device(0)
    try:
        sks = [O.interop_secret_key(i).to_bytes(32, "big") for i in range(n)]
        pks = dev.sk_to_pk(sks)
        sig, bad = dev.aggregate_signature_groups([dev.sign([sks[k] for k in committee], [msg] * size)])
        assert bad == [-1]
    finally:
        dev.close()
    (tmp_path / "pks.bin").write_bytes(b"".join(pks))
    (tmp_path / "spec.json").write_text(json.dumps({
        "active": active.tolist(), "increments": inc.tolist(), "epochSeed": epoch_seed.hex(), "startSlot": 96,
        "proposers": [-1 if p == SA.NONE else p for p in proposers], "seed": seed.hex(), "size": size,
        "committee": committee, "bits": (b"\xff" * (size // 8)).hex(), "msg": msg.hex(), "sig": sig[0].hex()}))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "gpu_sample.js"), str(tmp_path)],
                       capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert r.returncode == 0 and "gpu sample ok" in r.stdout, r.stdout + r.stderr
