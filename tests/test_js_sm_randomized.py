"""The JS verifiers forward `sameMessageRandomized` to the addon contexts they create
(tests/js/sm_randomized_host.js: a stand-in addon module, no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


def test_js_option_reaches_the_addon_contexts():
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "sm_randomized_host.js")], capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
