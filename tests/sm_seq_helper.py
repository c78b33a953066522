"""Cases of tests/test_gpu_sm_plan.py and tools/record_stage_sequences.py: one same-message
package per case, and the raw stage-name sequence it leaves once it has retired
(lb_last_stage_times, one entry per launch in launch order).

The package is three jobs of 1, 2 and 5 sets, the smallest at which the buffers of a package
(jobs, sets, the retry lists) all differ in size.  Every form of the call that adds or moves a
buffer is a case: the two aggregation modes, 96-byte keys, validator indices, indices mixed
with flagged key rows, the round-program decode on and off, an _agg call with a mask -- each
with every job valid (no phase 2) and ("retry") with the second signature of the 5-set job
signed over another root, so that job is retried set by set."""
import hashlib

import numpy as np

FIXTURE = "sm_stage_sequences.json"
JOB_SIZES = (1, 2, 5)
N_SETS = sum(JOB_SIZES)
SEED = hashlib.sha256(b"sm-plan").digest()
MASK = [[True], [False, True], [True, True, False, True, True]]

# name -> (environment, randomized mode, keys: "bytes" | "index" | "mixed", aggregate with MASK)
_FORMS = {
    "plain": ({}, False, "bytes", False),
    "randomized": ({}, True, "bytes", False),
    "index": ({}, False, "index", False),
    "mixed": ({}, False, "mixed", False),
    "lp_decode1": ({"LB_SM_LP_DECODE": "1"}, False, "bytes", False),
    "lp_decode0": ({"LB_SM_LP_DECODE": "0"}, False, "bytes", False),
    "agg_mask": ({}, False, "bytes", True),
}
CASES = {}
for _n, _f in _FORMS.items():
    CASES[_n] = _f + (False,)
    CASES[_n + ":retry"] = _f + (True,)


def workloads(device):
    """The keys, the two packages' signatures and roots, and per package the C oracle's verdict
    on every set alone (what a job's sets get: all true when its aggregate verifies, else each
    set's own), computed once."""
    from lodestar_amd.native import pack_blobs
    from oracle import bls12_381 as O
    from oracle import c_oracle as C
    sks = [O.interop_secret_key(i).to_bytes(32, "big") for i in range(N_SETS)]
    pks = device.sk_to_pk(sks)
    roots = [hashlib.sha256(b"sm-plan" + bytes([j])).digest() for j in range(len(JOB_SIZES))]
    msgs = [roots[j] for j, n in enumerate(JOB_SIZES) for _ in range(n)]
    sigs = device.sign(sks, msgs)
    bad = list(sigs)
    bad[4] = device.sign([sks[4]], [hashlib.sha256(b"sm-plan another root").digest()])[0]
    out = {"sks": sks, "pks": pks, "roots": roots}
    for name, s in (("valid", sigs), ("retry", bad)):
        blob, offs = pack_blobs(s)
        valid, _ = C.verify_requests(np.arange(N_SETS + 1, dtype=np.uint32), np.frombuffer(b"".join(pks), np.uint8),
                                     None, np.frombuffer(b"".join(msgs), np.uint8), blob, offs, SEED, threads=8)
        out[name] = (s, [bool(v) for v in valid])
    assert all(out["valid"][1]) and out["retry"][1] == [i != 4 for i in range(N_SETS)]
    return out


def _jobs(loads, keys, sigs):
    from lodestar_amd.native import LB_PK_ROW_FLAG
    jobs, v = [], 0
    for j, n in enumerate(JOB_SIZES):
        ix = range(v, v + n)
        if keys == "bytes":
            k = [loads["pks"][i] for i in ix]
        elif keys == "index":
            k = list(ix)
        else:  # even sets travel as rows of the package, odd sets by validator index
            k = [(LB_PK_ROW_FLAG | i) if i % 2 == 0 else i for i in ix]
        jobs.append((k, sigs[v:v + n], loads["roots"][j]))
        v += n
    return jobs


def run_case(name, loads):
    """-> (stage names in launch order, per-set verdicts, (job signatures, counts) or None)."""
    import os

    from lodestar_amd.native import Device
    env, randomized, keys, agg, retry = CASES[name]
    sigs = loads["retry" if retry else "valid"][0]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        dev = Device(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        if keys != "bytes":
            dev.pubkey_table_append(loads["pks"])
        dev.set_same_message_mode(randomized)
        rows = b"".join(loads["pks"]) if keys == "mixed" else None
        got = dev.verify_same_message_batch(_jobs(loads, keys, sigs), SEED, by_index=keys != "bytes", rows=rows,
                                            aggregate=agg, mask=MASK if agg else None)
        names = [n for n, _ in dev.last_stage_times(raw=True, limit=40)]
        return names, [v for job in got[0] for v in job], (got[2], got[3]) if agg else None
    finally:
        dev.close()
