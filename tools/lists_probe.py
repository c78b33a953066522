"""Index lists on the GPU, measured: the `shuffle` stage of lb_index_list_shuffle at
the reference benchmark's sizes, and one C4-shaped package (31,232 sets of ~17 keys from 2,048-bit
committees) through lb_verify_requests_async with flat pubkey_indices and through
lb_verify_requests_keys_async with set descriptors, alternating: the host's staging time of each
submission (LB_HOST_TRACE) and the expand_keys stage.  The signatures are one valid point repeated,
so the verdicts are false throughout: staging and expansion do not depend on them.

    python tools/lists_probe.py [tag] [out_dir]     -> out_dir/lists_probe_<tag>.json

A library without the keys entry points (LB_LIBRARY: an older build) runs the flat form alone."""
import json
import os
import re
import statistics
import sys
import time

import numpy as np

os.environ["LB_HOST_TRACE"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lodestar_amd.native import Device, load_library, pack_blobs  # noqa: E402

tag = sys.argv[1] if len(sys.argv) > 1 else "run"
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles")
os.makedirs(OUT, exist_ok=True)
lib = load_library()
has_keys = hasattr(lib, "lb_verify_requests_keys_async")
res = {"tag": tag, "has_keys": has_keys}
dev = Device(0)


def traced(fn):
    """run fn with fd 2 captured -> (result, lb_host_trace lines parsed)"""
    path = os.path.join(OUT, "trace_%s.tmp" % tag)
    sys.stderr.flush()
    saved = os.dup(2)
    with open(path, "w") as f:
        os.dup2(f.fileno(), 2)
        try:
            r = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
    rows = []
    for line in open(path):
        if line.startswith("lb_host_trace"):
            rows.append({k: float(v) for k, v in re.findall(r"(\w+)=([0-9.]+)", line)})
    return r, rows


if has_keys:
    sh = {}
    for n in (16384, 250000, 1048576, 4194304):
        active = np.arange(n, dtype=np.uint32)
        seed = bytes(range(32))
        st, wall, wall_noout = [], [], []
        for rep in range(9):
            t0 = time.perf_counter()
            dev.index_list_shuffle(0, active, seed)
            t1 = time.perf_counter()
            ms = dict(dev.last_stage_times())["shuffle"]
            t2 = time.perf_counter()
            dev.index_list_shuffle(0, active, seed, want_output=False)
            t3 = time.perf_counter()
            if rep >= 2:
                st.append(ms)
                wall.append((t1 - t0) * 1e3)
                wall_noout.append((t3 - t2) * 1e3)
        sh[n] = {"shuffle_stage_ms_median": statistics.median(st), "shuffle_stage_ms_min": min(st),
                 "shuffle_stage_ms_max": max(st), "call_wall_ms_median": statistics.median(wall),
                 "call_wall_no_readback_ms_median": statistics.median(wall_noout)}
        print("shuffle", n, sh[n], flush=True)
    res["shuffle"] = sh

# ---- the C4-shaped package: 31,232 sets of ~17 keys from 2,048-bit committees ----
NS, PER_REQ, COMM, NLIST, NTAB = 31232, 128, 2048, 65536, 4096
rnd = np.random.default_rng(4)
sks = [int(x).to_bytes(32, "big") for x in rnd.integers(1, 2 ** 62, NTAB)]
pks = dev.sk_to_pk(sks)
dev.pubkey_table_append(pks)
lst = rnd.integers(0, NTAB, NLIST).astype(np.uint32)
if has_keys:
    dev.index_list_put(1, lst)
one_sig = dev.sign(sks[:1], [bytes(32)])[0]
sigs = [one_sig] * NS
blob, offs = pack_blobs(sigs)
msgs = rnd.integers(0, 256, NS * 32).astype(np.uint8)
req_off = np.arange(0, NS + 1, PER_REQ, dtype=np.uint32)
bits = np.zeros((NS, COMM // 8), np.uint8)
set_keys = np.zeros((NS, 5), np.uint32)
idx, pk_off = [], [0]
for s in range(NS):
    k = int(rnd.integers(12, 23))
    pos = np.sort(rnd.choice(COMM, k, replace=False))
    np.bitwise_or.at(bits[s], pos >> 3, (1 << (pos & 7)).astype(np.uint8))
    start = (s % (NLIST // COMM)) * COMM
    set_keys[s] = (2, 1, start, COMM, s * (COMM // 8))
    idx.append(lst[start + pos])
    pk_off.append(pk_off[-1] + k)
idx = np.concatenate(idx).astype(np.uint32)
pk_off = np.array(pk_off, np.uint32)
bits_flat = bits.reshape(-1)
res["c4"] = {"sets": NS, "n_keys": int(pk_off[-1]), "flat_key_bytes": int(4 * pk_off[-1] + 4 * (NS + 1)),
             "descriptor_bytes": int(20 * NS + len(bits_flat))}
seed = bytes(32)


def run_flat():
    pc = dev.verify_requests_async(req_off, None, pk_off, msgs, blob, offs, seed, pk_indices=idx)
    return dev.wait_call(pc)


def run_keys():
    pc = dev.verify_requests_keys_async(req_off, set_keys, None, bits_flat, msgs, blob, offs, seed)
    return dev.wait_call(pc)


forms = [("flat", run_flat)] + ([("keys", run_keys)] if has_keys else [])
acc = {name: {"stage": [], "check": [], "finish": [], "pipeline": [], "total": [], "expand_keys": [], "device_ms": []}
       for name, _ in forms}
verdicts = {}
for rep in range(9):  # alternating, 2 warm-up rounds
    for name, fn in forms:
        r, rows = traced(fn)
        verdicts[name] = (r.valid.tolist(), r.errors.tolist(), r.set_status.tolist())
        if rep < 2:
            continue
        row = rows[-1]
        a = acc[name]
        a["check"].append(row["check"])
        a["finish"].append(row["finish_slot"])
        a["stage"].append(row["stage"] - row["finish_slot"])  # the staging proper (+ the keys' count)
        a["pipeline"].append(row["pipeline"] - row["stage"])
        a["total"].append(row["total"])
        a["device_ms"].append(r.device_ms)
        a["expand_keys"].append(dict(dev.last_stage_times()).get("expand_keys", 0.0))
if has_keys:
    res["c4"]["same_verdicts"] = verdicts["flat"] == verdicts["keys"]
for name, a in acc.items():
    res["c4"][name] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in a.items()}
    print("c4", name, res["c4"][name], flush=True)
os.remove(os.path.join(OUT, "trace_%s.tmp" % tag))
json.dump(res, open(os.path.join(OUT, "lists_probe_%s.json" % tag), "w"), indent=1)
dev.close()
print("lists_probe ok", tag)
