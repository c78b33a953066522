#!/usr/bin/env python3
"""Record tests/golden/pipeline_stage_sequences.json: the raw stage-name sequence of one
pipeline call per case of tests/pipe_seq_helper.py, on an MI355X.  tests/test_gpu_pipe_plan.py
holds the pipeline to it, so record it on the commit whose launch order is the reference
(before a change that must keep the order), never to make a failing test pass.
--sm records tests/golden/sm_stage_sequences.json instead: one same-message package per case
of tests/sm_seq_helper.py, for tests/test_gpu_sm_plan.py.

  python tools/record_stage_sequences.py [--sm] [OUT.json]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from lodestar_amd.native import Device
    argv = [a for a in sys.argv[1:] if a != "--sm"]
    sm = len(argv) != len(sys.argv) - 1
    if sm:
        from tests import sm_seq_helper as H
    else:
        from tests import pipe_seq_helper as H
    out = argv[0] if argv else os.path.join(ROOT, "tests", "golden", H.FIXTURE)
    dev = Device(0)
    loads = H.workloads(dev)
    dev.close()
    rec = {}
    for name in H.CASES:
        if sm:
            names, valid, _ = H.run_case(name, loads)
            ok = valid == loads["retry" if H.CASES[name][-1] else "valid"][1]
        else:
            names, valid, err = H.run_case(name, loads)
            want = loads[H.CASES[name][1]]
            ok = valid == want[2] and err == want[3]
        if not ok:
            raise SystemExit("%s: verdicts differ from the C oracle's: %s" % (name, valid))
        rec[name] = names
        print(name, len(names), " ".join(names), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
