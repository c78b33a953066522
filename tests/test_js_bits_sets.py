"""Sets of type "bits" on the JS host (tests/js/test_bits_sets.js, a mock backend under node):
descriptor packing, the fallback to today's form, syncShuffling / putIndexList; and the addon's
marshalling of the keys form and of the index-list calls."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "lodestar_amd", "napi", "lodestar_bls.node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


def test_js_bits_sets_packing():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "test_bits_sets.js")], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode == 0 and "0 failed" in r.stdout, r.stdout + r.stderr


def test_addon_exports_the_list_calls():
    if not os.path.exists(ADDON):
        from lodestar_amd.napi import build as nb
        if not nb.available():
            pytest.skip("node headers not available")
        nb.build()
    script = ("const a = require(%r); const p = a.Context.prototype;"
              "if (typeof p.indexListPut !== 'function' || typeof p.indexListShuffle !== 'function') process.exit(3);"
              "console.log('list calls ok');" % ADDON)
    r = subprocess.run([NODE, "-e", script], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert r.returncode == 0 and "list calls ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_addon_bits_sets_on_the_gpu(tmp_path):
    """Index lists and bits sets through the real addon (tests/js/gpu_bits_sets.js): the keys,
    signatures and the expected shuffling come from here."""
    import hashlib
    import json
    import sys

    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import shuffle_helper as SH
    from lodestar_amd.native import Device
    from oracle import bls12_381 as O
    n = 48
    rnd = np.random.default_rng(9)
    active = rnd.permutation(n)[:40].astype(np.uint32)
    seed = hashlib.sha256(b"js-epoch").digest()
    shuffling = SH.unshuffle_rounds(active, seed)
    sync = rnd.integers(0, n, 64).astype(np.uint32)
    lists = {0: shuffling, 1: sync}
    sets = []
    for i in range(6):
        lid = i % 2
        start, length = (8 * i, 8) if lid == 0 else (3 * i, 30)
        flags = rnd.integers(0, 2, length).astype(np.uint8)
        flags[0] = flags[1] = 1  # (two participants at least: clearing one leaves a non-empty set)
        bits = np.packbits(flags, bitorder="little").tobytes()
        sets.append({"kind": "bits", "list": lid, "start": start, "length": length, "bits": bits.hex(),
                     "keys": [int(lists[lid][start + j]) for j in range(length) if flags[j]]})
    sets.insert(1, {"kind": "single", "index": 7, "keys": [7]})
    sets.append({"kind": "aggregate", "indices": [3, 3, 9], "keys": [3, 3, 9]})
    dev = Device(0)
    try:
        sks = [O.interop_secret_key(i).to_bytes(32, "big") for i in range(n)]
        pks = dev.sk_to_pk(sks)
        for i, s in enumerate(sets):
            msg = hashlib.sha256(b"js-bits" + bytes([i])).digest()
            sig, bad = dev.aggregate_signature_groups([dev.sign([sks[k] for k in s["keys"]], [msg] * len(s["keys"]))])
            assert bad == [-1]
            s["msg"], s["sig"] = msg.hex(), sig[0].hex()
    finally:
        dev.close()
    (tmp_path / "pks.bin").write_bytes(b"".join(pks))
    (tmp_path / "spec.json").write_text(json.dumps({"active": active.tolist(), "seed": seed.hex(),
                                                    "shuffling": shuffling.tolist(), "sync": sync.tolist(),
                                                    "sets": sets}))
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "gpu_bits_sets.js"), str(tmp_path)],
                       capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert r.returncode == 0 and "gpu bits sets ok" in r.stdout, r.stdout + r.stderr
