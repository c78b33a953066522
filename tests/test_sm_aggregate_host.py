"""Per-job aggregate signatures of same-message packages, without a GPU: the C ABI's new
entry points exist and refuse misuse, the Python restatement (tests/sm_agg_helper.py) agrees
with hand-built sums, and the Python and JS verifiers carry `include` down and the results up
through stand-in backends."""
import asyncio
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sm_agg_helper as A  # noqa: E402
from lodestar_amd import native  # noqa: E402
from oracle import bls12_381 as O  # noqa: E402

NEW = ("lb_verify_same_message_batch_agg", "lb_verify_same_message_batch_agg_async", "lb_aggregate_signature_groups")


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "lodestar_bls.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(native.library_path())
    for name in NEW:
        assert re.search(r"^\s*int\s+%s\s*\(" % name, code, flags=re.M), name
        assert name in native.EXPORTED_SYMBOLS
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+LB_AGG_NO_CHECK\s+1u", code)
    # the one semantic trap is stated where the call is declared
    assert "cancelling pair" in src and "masked subset" in src


def test_null_ctx_is_refused():
    lib = native.load_library()
    b = native._SameMessageBatch(0, 0, None, None, None, None, None, None, None)
    t = ctypes.c_uint64(0)
    assert lib.lb_verify_same_message_batch_agg(None, ctypes.byref(b), None, None, None, None, None,
                                                None) == native.LB_ERR_INVALID_ARGUMENT
    assert lib.lb_verify_same_message_batch_agg_async(None, ctypes.byref(b), None, None, None, None, None,
                                                      ctypes.byref(t)) == native.LB_ERR_INVALID_ARGUMENT
    off = np.zeros(2, np.uint32)
    out = np.zeros(96, np.uint8)
    bad = np.zeros(1, np.int32)
    assert lib.lb_aggregate_signature_groups(None, 1, off.ctypes.data, out.ctypes.data, off.ctypes.data, 0,
                                             out.ctypes.data, bad.ctypes.data) == native.LB_ERR_INVALID_ARGUMENT


def test_helper_against_hand_built_sums():
    p = O.g2_mul(O.G2, 5)
    sp, sn = O.g2_to_bytes(p), O.g2_to_bytes(O.E2.neg(p))
    assert A.INFINITY96 == bytes([0xC0]) + bytes(95) == native.G2_INFINITY_COMPRESSED
    # P + (-P): the infinity encoding, still a count of two
    jobs = [(None, [sp, sn], None)]
    assert A.expected_job_aggregates(jobs, [[True, True]]) == [(A.INFINITY96, 2)]
    # [2]G + [3]G + [7]G = [12]G
    sigs = [O.g2_to_bytes(O.g2_mul(O.G2, k)) for k in (2, 3, 7)]
    assert A.aggregate_bytes(sigs) == O.g2_to_bytes(O.g2_mul(O.G2, 12))
    jobs = [(None, sigs, None), (None, [], None)]
    # verdicts and mask both select: set 1 invalid, set 2 masked out -> [2]G alone
    got = A.expected_job_aggregates(jobs, [[True, False, True], []], [[True, True, False], []])
    assert got == [(O.g2_to_bytes(O.g2_mul(O.G2, 2)), 1), (A.INFINITY96, 0)]
    sums, bad = A.expected_groups([sigs[:2], [sigs[2], bytes([10]) * 96], [sigs[0]]])
    assert bad == [-1, 3, -1]
    assert sums == [O.g2_to_bytes(O.g2_mul(O.G2, 5)), bytes(96), sigs[0]]


class FakeDev:
    """Stand-in for native.Device (no GPU): every set valid but those whose signature starts with
    0xff; the "aggregate" of a job is a tag of what was summed, so the test sees the mask."""

    def __init__(self):
        self.calls = []
        self.last_stats = (0, 0)
        self.last_device_ms = 0.0

    def verify_same_message_batch_async(self, jobs, seed, by_index=False, aggregate=False, mask=None):
        self.calls.append({"n_jobs": len(jobs), "aggregate": aggregate, "mask": mask})
        pc = native.PendingSameMessage(0, len(jobs), None, None, np.zeros(1, np.uint32), list(jobs))
        if aggregate:
            pc.sig96 = np.zeros(1, np.uint8)
            pc.count = mask
        return pc

    def wait_same_message(self, pc):
        jobs = pc.keep
        res = [[s[0] != 0xFF for s in sigs] for _, sigs, _ in jobs]
        fast = [all(r) for r in res]
        if pc.sig96 is None:
            return res, fast, (0, 0), 0.0
        mask = pc.count
        sums, counts = [], []
        for j, (_, sigs, _) in enumerate(jobs):
            take = [i for i in range(len(sigs)) if res[j][i] and (mask is None or mask[j][i])]
            sums.append(bytes([len(take)]) + bytes(take).ljust(95, b"\0"))
            counts.append(len(take))
        return res, fast, sums, counts

    def last_stage_times(self):
        return []

    def close(self):
        pass


def test_python_verifiers_carry_include_and_results():
    from lodestar_amd.verifier import BlsGpuSingleThreadVerifier, BlsGpuVerifier, DeviceBackend, PublicKey

    def sets(n, bad=()):
        return [(PublicKey(bytes([7]) * 96), bytes([0xFF if i in bad else 1]) * 96) for i in range(n)]

    async def main():
        dev = FakeDev()
        v = BlsGpuVerifier(backends=[DeviceBackend(seed_source=lambda: bytes(32), dev=dev, capacity=2)])
        # 200 sets stay ONE job (no chunking to 128): one aggregate; set 3 invalid, set 5 masked
        inc = [i != 5 for i in range(200)]
        big = v.verify_and_aggregate_same_message(sets(200, bad=(3,)), bytes(32), include=inc)
        plain = v.verify_signature_sets_same_message(sets(2), bytes([1]) * 32)
        none = v.verify_and_aggregate_same_message(sets(2, bad=(0, 1)), bytes([2]) * 32)
        r_big, r_plain, r_none = await asyncio.gather(big, plain, none)
        await v.close()
        return dev, r_big, r_plain, r_none
    dev, r_big, r_plain, r_none = asyncio.run(main())
    # the three jobs shared one device call, an aggregate one, with one mask row per job
    assert len(dev.calls) == 1 and dev.calls[0]["n_jobs"] == 3 and dev.calls[0]["aggregate"] is True
    assert dev.calls[0]["mask"] == [[i != 5 for i in range(200)], [True, True], [True, True]]
    valid, sig, count = r_big
    assert valid == [i != 3 for i in range(200)] and count == 198
    assert sig[0] == 198 and sig[1:5] == bytes([0, 1, 2, 4]) and 5 not in sig[1:7]
    assert r_plain == [True, True]  # a plain job beside them: its result keeps its shape
    assert r_none == ([False, False], None, 0)  # nothing summed: no signature

    # a package without an aggregate job is submitted exactly as before
    async def plain_only():
        dev = FakeDev()
        v = BlsGpuVerifier(backends=[DeviceBackend(seed_source=lambda: bytes(32), dev=dev, capacity=2)])
        out = await v.verify_signature_sets_same_message(sets(3), bytes(32))
        await v.close()
        return dev, out
    dev, out = asyncio.run(plain_only())
    assert out == [True, True, True] and dev.calls == [{"n_jobs": 1, "aggregate": False, "mask": None}]

    async def single():
        dev = FakeDev()
        st = BlsGpuSingleThreadVerifier(DeviceBackend(seed_source=lambda: bytes(32), dev=dev, capacity=1))
        out = await st.verify_and_aggregate_same_message(sets(4, bad=(2,)), bytes(32), include=[True, False, True, True])
        await st.close()
        return dev, out
    dev, (valid, sig, count) = asyncio.run(single())
    assert dev.calls == [{"n_jobs": 1, "aggregate": True, "mask": [[True, False, True, True]]}]
    assert valid == [True, True, False, True] and count == 2 and sig[:3] == bytes([2, 0, 3])


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_verifiers_pass_the_flag_and_mask_and_shape_the_result():
    r = subprocess.run([shutil.which("node"), os.path.join(ROOT, "tests", "js", "sm_aggregate_host.js")],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
