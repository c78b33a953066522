"""Cases of tests/test_gpu_pipe_plan.py and tools/record_stage_sequences.py: one pipeline call
per case, under the case's switches, and the raw stage-name sequence it leaves
(lb_last_stage_times, one entry per launch in launch order).

The small workload is 130 single-key sets in requests of 1, 2 and 127 sets (a one-set
request, a request below and one above a lane's 68 lines) with the latency path off; "bad"
replaces one set's message.  Three requests stay below LB_MERGE_MIN's default, so every
switch of the merged check is also run with LB_MERGE_MIN=1 (the "merged:" cases)."""
import hashlib

import numpy as np

FIXTURE = "pipeline_stage_sequences.json"
N_SMALL, SMALL_REQ = 130, (0, 1, 3, 130)
N_LONE = 1000

_SWITCHES = [
    ("default", {}, False),
    ("msm", {"LB_MSM_MIN": "1"}, False),
    ("msm_mtail0", {"LB_MSM_MIN": "1", "LB_MTAIL": "0"}, False),
    ("pairs_split0", {"LB_ACC": "pairs", "LB_ACC_SPLIT": "0"}, False),
    ("pairs_split1", {"LB_ACC": "pairs", "LB_ACC_SPLIT": "1"}, False),
    ("level0", {"LB_LEVEL": "0"}, False),
    ("rtail0_bad", {"LB_RTAIL": "0"}, True),
    ("step_split1", {"LB_STEP_SPLIT": "1"}, False),
    ("step_split4", {"LB_STEP_SPLIT": "4"}, False),
    ("lp_stages_off", {"LB_LP_DECODE": "0", "LB_LP_HASH_FINISH": "0", "LB_LP_LINES": "0"}, False),
]

# name -> (environment, workload, how it is submitted)
CASES = {}
for _n, _e, _bad in _SWITCHES:
    CASES[_n] = (dict(_e, LB_MILLER="lines"), "small_bad" if _bad else "small", "sync")
    CASES["merged:" + _n] = (dict(_e, LB_MILLER="lines", LB_MERGE_MIN="1"), "small_bad" if _bad else "small", "sync")
CASES["merge_min0"] = ({"LB_MILLER": "lines", "LB_MERGE_MIN": "0"}, "small", "sync")
CASES["merged:pairs_msm"] = ({"LB_MILLER": "lines", "LB_MERGE_MIN": "1", "LB_ACC": "pairs", "LB_MSM_MIN": "1"},
                             "small", "sync")
CASES["merged:bad"] = ({"LB_MILLER": "lines", "LB_MERGE_MIN": "1", "LB_MSM_MIN": "1"}, "small_bad", "sync")
CASES["miller_lane"] = ({"LB_MILLER": "lane"}, "small", "sync")
CASES["miller_wave"] = ({"LB_MILLER": "wave"}, "small", "sync")
CASES["lone_1000"] = ({}, "lone", "lone")
CASES["two_phase"] = ({"LB_MILLER": "lines"}, "small", "two_phase")


def _workload(device, n, req_off, tag, bad=None):
    from lodestar_amd.native import pack_blobs
    from oracle import bls12_381 as O
    sks = [O.interop_secret_key(i).to_bytes(32, "big") for i in range(n)]
    msgs = [hashlib.sha256(tag + i.to_bytes(4, "little")).digest() for i in range(n)]
    pks = device.sk_to_pk(sks)
    sigs = device.sign(sks, msgs)
    if bad is not None:
        msgs[bad] = bytes(32)
    blob, offs = pack_blobs(sigs)
    return (np.array(req_off, np.uint32), np.frombuffer(b"".join(pks), np.uint8), None,
            np.frombuffer(b"".join(msgs), np.uint8), blob, offs)


def workloads(device):
    """The three workloads and the C oracle's verdicts for each, computed once."""
    from oracle import c_oracle as C
    seed = hashlib.sha256(b"pipe-plan").digest()
    out = {}
    for name, args in (("small", _workload(device, N_SMALL, SMALL_REQ, b"pp")),
                       ("small_bad", _workload(device, N_SMALL, SMALL_REQ, b"pp", bad=77)),
                       ("lone", _workload(device, N_LONE, (0, N_LONE), b"pl"))):
        valid, err = C.verify_requests(*args, seed, threads=16)
        out[name] = (args, seed, [int(v) for v in valid], [int(e) for e in err])
    return out


def run_case(name, loads):
    """-> (stage names in launch order, verdicts, rejection codes) of the case's one call."""
    import os

    from lodestar_amd.native import Device
    env, load, how = CASES[name]
    args, seed = loads[load][:2]
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
        if how != "lone":
            dev.set_latency_path(0)
        if how == "two_phase":
            pc = dev.verify_requests_async(*args, seed, partial=True)
            ok = dev.gt_check([dev.partial_wait(pc)])
            dev.verify_finish(pc, ok)
            res = dev.wait_call(pc)
        else:
            res = dev.verify_requests(*args, seed)
        names = [n for n, _ in dev.last_stage_times(raw=True, limit=40)]
        return names, [int(v) for v in res.valid], [int(e) for e in res.errors]
    finally:
        dev.close()
