"""Cost of the per-job aggregate signatures of a same-message package.

Two packages by validator index in the plain mode -- 512 jobs x 128 sets (the bench's
same-message shape) and 4,096 jobs x 4 sets -- each submitted 23 times (3 warm-ups) as
lb_verify_same_message_batch_async and as lb_verify_same_message_batch_agg_async: device_ms of
both, and the stages sm_aggregate / sm_job_sig / sm_decode from lb_last_stage_times (median, min,
max).  --plain-only: the plain call alone (also runs against a tree without the _agg entry
points, e.g. the parent commit's, for the before / after of device_ms).

    python tools/sm_job_sig_probe.py [--plain-only] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import workloads as W  # noqa: E402
from lodestar_amd import native  # noqa: E402

SHAPES = (("512x128", 512, 128), ("4096x4", 4096, 4))
CALLS, WARMUP = 23, 3


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    # (a 4,096-job package's pipeline alone is 35 launches; sm_job_sig comes behind them)
    more = {} if a.plain_only else {"limit": 40}
    dev = native.Device(0)
    keys = W.make_keys(dev, 16384)
    dev.pubkey_table_append(keys.pks)
    out = {"library": native.library_path()}
    for name, nj, per in SHAPES:
        jobs, _ = W.same_message_jobs(dev, keys, n_jobs=nj, per_job=per)
        r = {}
        for label, agg in (("plain", False),) + (() if a.plain_only else (("agg", True),)):
            ms, stages = [], []
            for _ in range(CALLS):
                if agg:
                    dev.wait_same_message(dev.verify_same_message_batch_async(jobs, bytes(32), by_index=True,
                                                                              aggregate=True))
                    ms.append(dev.last_device_ms)
                else:
                    ms.append(dev.wait_same_message(dev.verify_same_message_batch_async(jobs, bytes(32),
                                                                                        by_index=True))[3])
                stages.append(dict(dev.last_stage_times(**more)))
            ms, stages = ms[WARMUP:], stages[WARMUP:]
            r[label] = {"device_ms": spread(ms), "launches": len(dev.last_stage_times(raw=True, **more))}
            for st in ("sm_aggregate", "sm_job_sig", "sm_decode"):
                v = [s[st] for s in stages if st in s]
                if v:
                    r[label][st] = spread(v)
        out[name] = r
        print(name, json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    dev.close()


if __name__ == "__main__":
    main()
