"""The N-API addon's scheduling without a GPU: the real addon.cc, built with its usual flags
against a stand-in for liblodestar_bls.so (tests/native/lb_stub.c: every lb_* call logged,
canned outputs), driven under node by tests/js/addon_sched.js.  Priority order, the capacity
bound, mirroring into the latency lane, lane retirement, partial -> finish, close and every
method's result shape are asserted from the stub's log and the resolved values."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")

pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


@pytest.fixture(scope="module")
def stub_addon(tmp_path_factory):
    from lodestar_amd.napi import build as nb
    if not nb.available() or shutil.which("gcc") is None:
        pytest.skip("node headers not available")
    d = tmp_path_factory.mktemp("addon_stub")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror",
                           os.path.join(ROOT, "tests", "native", "lb_stub.c"), "-o", str(d / "liblodestar_bls.so")])
    return nb.build(force=True, out=str(d / "lodestar_bls.node"), lib_dir=str(d)), d


def test_stub_defines_what_the_addon_references(stub_addon):
    """The stub is exactly the addon's view of the C ABI: no entry point missing (the addon would
    not load), none left over from an operation that is gone."""
    import re
    src = open(os.path.join(ROOT, "lodestar_amd", "napi", "addon.cc")).read()
    used = set(re.findall(r"\b(lb_[a-z0-9_]+)\(", src))
    out = subprocess.check_output(["nm", "-D", "--defined-only", str(stub_addon[1] / "liblodestar_bls.so")], text=True)
    defined = {m for m in re.findall(r"\bT (lb_[a-z0-9_]+)", out)}
    assert defined == used


def test_addon_scheduling(stub_addon, tmp_path):
    addon, _ = stub_addon
    r = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "addon_sched.js"), addon, str(tmp_path)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "addon sched ok" in r.stdout
