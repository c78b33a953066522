#!/usr/bin/env python3
"""Record tests/golden/pipeline_stage_sequences.json: the raw stage-name sequence of one
pipeline call per case of tests/pipe_seq_helper.py, on an MI355X.  tests/test_gpu_pipe_plan.py
holds the pipeline to it, so record it on the commit whose launch order is the reference
(before a change that must keep the order), never to make a failing test pass.

  python tools/record_stage_sequences.py [OUT.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from lodestar_amd.native import Device
    from tests import pipe_seq_helper as H
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", H.FIXTURE)
    dev = Device(0)
    loads = H.workloads(dev)
    dev.close()
    rec = {}
    for name in H.CASES:
        names, valid, err = H.run_case(name, loads)
        want = loads[H.CASES[name][1]]
        if valid != want[2] or err != want[3]:
            raise SystemExit("%s: verdicts differ from the C oracle's: %s %s" % (name, valid, err))
        rec[name] = names
        print(name, len(names), " ".join(names), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
