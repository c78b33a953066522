"""Balance-weighted sampling on the GPU, measured: the `sample` stage of
lb_sample_by_balance (device events) and the host clock around the call, median of 7 after 2
warm-ups, for the two shapes the node has --

    proposers   32 seeds, count 1, max_candidates n        (computeProposers)
    committee   1 seed, count 512, stored as an index list (getNextSyncCommitteeIndices)

at n = 16,384 / 250,000 / 1,048,576 active validators whose increments are all 32 (every
candidate is accepted), plus the committee at acceptance 1/4 (increments 8), where the walk takes
a second pass.

    python tools/sample_probe.py [tag] [out_dir]     -> out_dir/sample_probe_<tag>.json"""
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lodestar_amd.native import Device  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "run"
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
os.makedirs(OUT, exist_ok=True)
dev = Device(0)
res = {"tag": tag, "shapes": {}}
epoch_seed = bytes(range(32))
slot_seeds = [hashlib.sha256(epoch_seed + i.to_bytes(8, "little")).digest() for i in range(32)]
for n in (16384, 250000, 1048576):
    active = np.arange(n, dtype=np.uint32)
    for name, inc, seeds, count, cap, store in (("proposers", 32, slot_seeds, 1, n, 0xFFFFFFFF),
                                                ("committee", 32, [epoch_seed], 512, 1 << 22, 3),
                                                ("committee_quarter", 8, [epoch_seed], 512, 1 << 22, 3)):
        dev.balance_table_put(np.full(n, inc, np.uint8))
        stage, wall, tried = [], [], None
        for rep in range(9):
            t0 = time.perf_counter()
            r = dev.sample_by_balance(seeds, count, active, 32, cap, store_list=store)
            t1 = time.perf_counter()
            if rep >= 2:
                stage.append(dict(dev.last_stage_times())["sample"])
                wall.append((t1 - t0) * 1e3)
            tried = r.tried.tolist()
        assert r.found.tolist() == [count] * len(seeds)
        row = {"sample_stage_ms_median": statistics.median(stage), "sample_stage_ms_min": min(stage),
               "sample_stage_ms_max": max(stage), "call_wall_ms_median": statistics.median(wall),
               "call_wall_ms_min": min(wall), "tried_max": max(tried)}
        res["shapes"]["%s_%d" % (name, n)] = row
        print(name, n, row, flush=True)
json.dump(res, open(os.path.join(OUT, "sample_probe_%s.json" % tag), "w"), indent=1)
dev.close()
print("sample_probe ok", tag)
