"""The carving of the host calls' buffers (lodestar_amd/csrc/bls_carve.h) on the host: a g++ build
of the header behind ctypes (tests/native/carve_host.cpp).  The primitive on random declaration
lists; the same-message layout over a grid of packages, its sizes restated by hand here; the
host-buffer call's and the latency path's lists; the capacity rule of the context's device arrays
(dev_array_cap).  A stand-alone build of the same file walks
the grid under -fsanitize=address,undefined where the host compiler has the runtime."""
import ctypes
import itertools
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "carve_host.cpp")
with open(os.path.join(ROOT, "lodestar_amd", "csrc", "bls_lp.h")) as _f:
    DEC_MAX = int(re.search(r"#define LB_SM_DEC_MAX (\d+)", _f.read()).group(1))

ULL, LL = ctypes.c_ulonglong, ctypes.c_longlong


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("carve") / "libcarve_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC])
    L = ctypes.CDLL(out)
    L.cv_carve.restype = ULL
    L.cv_carve.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ULL, ULL] + [ctypes.c_void_p] * 3
    L.cv_sm_name.restype = ctypes.c_char_p
    L.cv_sm_layout.argtypes = [ctypes.c_uint] * 3 + [ctypes.c_int] * 4 + [ULL, ctypes.c_void_p, ctypes.c_void_p]
    L.cv_lp_layout.restype = ULL
    L.cv_lp_layout.argtypes = [ULL, ctypes.c_int, ULL, ctypes.c_void_p]
    L.cv_lp_ws_bytes.restype = ULL
    L.cv_lp_ws_bytes.argtypes = [ULL]
    L.cv_host_layout.restype = ULL
    L.cv_host_layout.argtypes = [ctypes.c_uint, ctypes.c_uint, ULL, ULL, ctypes.c_uint, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_void_p]
    L.cv_dev_array_cap.restype = L.cv_dev_array_max.restype = ctypes.c_uint
    L.cv_dev_array_cap.argtypes = [ctypes.c_uint] * 3 + [ctypes.c_int]
    return L


def al(x):
    return (x + 255) // 256 * 256


def check_run(bufs, start=0):
    """bufs: (name, offset or -1, bytes) in layout order -> the end: aligned, increasing, disjoint."""
    end = start
    for name, off, size in bufs:
        if off < 0:
            continue
        assert off % 256 == 0 and off >= end and off < end + 256, (name, off, end)
        end = off + size
    return end


# ---- the primitive -------------------------------------------------------------------------------
def carve(lib, decls, start=0, cap=None):
    n = len(decls)
    arr = lambda t, v: (t * max(n, 1))(*v)  # noqa: E731
    off, addr, fits = (LL * max(n, 1))(), (LL * max(n, 1))(), ctypes.c_int(0)
    args = [arr(ctypes.c_int, [d[0] for d in decls]), arr(ctypes.c_int, [d[1] for d in decls]),
            arr(ULL, [d[2] for d in decls]), arr(ctypes.c_int, [d[3] for d in decls])]
    end = lib.cv_carve(n, *args, start, (1 << 62) if cap is None else cap, off, addr, ctypes.byref(fits))
    return end, list(off)[:n], list(addr)[:n], bool(fits.value)


def test_primitive_random_lists(lib):
    rng = random.Random(20240)
    for _ in range(300):
        n = rng.randrange(0, 25)
        decls = [(rng.randrange(3), rng.choice((1, 4, 8, 144)), rng.choice((0, 0, 1, 3, 64, 65, 257, 100000)),
                  rng.random() < 0.75) for _ in range(n)]
        start = rng.choice((0, 0, 7, 256, 1000))
        end, off, addr, fits = carve(lib, decls, start)
        assert fits
        bufs = [("%d" % i, off[i], d[1] * d[2]) for i, d in enumerate(decls)]
        assert end == check_run(bufs, start)  # the total is the end of the last present buffer
        for i, d in enumerate(decls):
            assert (off[i] >= 0) == bool(d[3])
            assert addr[i] == off[i]  # bound to base + offset; an absent buffer to nullptr
        assert carve(lib, decls, start, cap=end)[3]
        if end:
            assert not carve(lib, decls, start, cap=end - 1)[3]


def test_primitive_refuses_a_list_longer_than_its_capacity(lib):
    decls = [(1, 1, 1, True)] * 25
    assert not carve(lib, decls)[3] and carve(lib, decls[:24])[3]


# ---- the same-message layout ---------------------------------------------------------------------
JOBS = [1, 2, 3, 257]
SETS = [0, 1, DEC_MAX, DEC_MAX + 1, 5000]


def sm_layout(lib, nj, ns, rows, by_index, agg, nr=None, front_only=False):
    n = lib.cv_sm_count()
    out, p12 = (LL * n)(), (ULL * 2)()
    lib.cv_sm_layout(nj, ns, rows, by_index, agg, int(0 < ns <= DEC_MAX), front_only, ns if nr is None else nr, out, p12)
    return {lib.cv_sm_name(i).decode(): out[i] for i in range(n)}, p12[0], p12[1]


def sm_sizes(nj, ns, rows, by_index, nr):
    """Bytes of every buffer of the layout, by hand (bls_host.hip's kernels read and write these)."""
    ns1 = max(ns, 1)
    inputs = [("joff", 4 * (nj + 1)), ("pk", ns * (4 if by_index else 96)), ("sigo", 4 * (ns + 1)), ("sig", 96 * ns),
              ("msg", 32 * nj), ("seed", 32), ("areq", 4 * (nj + 1)), ("asig", 4 * (nj + 1)), ("rows", 96 * rows)]
    phase1 = [("d_sig", 288 * ns1), ("d_sst", ns1), ("d_jpk", 144 * nj), ("d_jpkst", nj), ("d_pk96", 96 * nj),
              ("d_sig192", 192 * nj), ("d_jbad", nj), ("d_valid", nj), ("d_err", nj), ("d_mask", ns1), ("d_inc", ns1),
              ("d_agg96", 96 * nj), ("d_aggcnt", 4 * nj)]
    dec = [("dec_in", 256 * ns), ("dec_fl", 12 * ns), ("dec_out", 128 * ns), ("dec_ofl", 8 * ns), ("dec_pre", ns)]
    phase2 = [("d_rset", 8 * ns), ("d_rsig", 288 * nr), ("d_rst", nr), ("d_rmsg", 32 * nr), ("d_ridx", 4 * nr),
              ("d_rreq", 4 * (nr + 1)), ("d_rvalid", nr), ("d_rerr", nr)]
    pinned = [("h_valid", nj), ("h_err", nj), ("h_jbad", nj), ("h_jpkst", nj), ("h_rset", 8 * ns1), ("h_rvalid", ns1),
              ("h_rerr", ns1), ("h_mask", ns1), ("h_agg96", 96 * nj), ("h_aggcnt", 4 * nj)]
    return inputs, phase1, dec, phase2, pinned


@pytest.mark.parametrize("rows,by_index,agg", [(r, i, a) for r, i, a in itertools.product((0, 3), (0, 1), (0, 1))
                                               if i or not r])
def test_same_message_grid(lib, rows, by_index, agg):
    totals = {}
    for nj, ns in itertools.product(JOBS, SETS):
        L, p1, p2 = sm_layout(lib, nj, ns, rows, by_index, agg)
        inputs, phase1, dec, phase2, pinned = sm_sizes(nj, ns, rows, by_index, ns)
        run = lambda bufs, start=0: check_run([(n, L[n], z) for n, z in bufs], start)  # noqa: E731
        # complete: what the package has is there, what it has not is absent
        have = {n for n, v in L.items() if v >= 0}
        absent = ({"rows"} if not rows else set()) | (set() if agg else {"d_mask", "d_inc", "d_agg96", "d_aggcnt",
                                                                          "h_mask", "h_agg96", "h_aggcnt"})
        absent |= set() if 0 < ns <= DEC_MAX else {n for n, _ in dec}
        assert have == set(L) - absent
        # the slab: inputs, phase 1's buffers, its pipeline; behind it the decode records and phase 2
        assert L["in_bytes"] == al(run(inputs))
        assert L["pipe1"] == run(phase1, L["in_bytes"])
        late = L["pipe1"] + p1
        dec_end = run(dec, late)
        assert L["pipe2"] == run(phase2, late)
        assert L["ws_end"] == max(dec_end, L["pipe2"] + p2)
        # the pinned area: the inputs, then every result region
        assert L["pin_end"] == run(pinned, L["in_bytes"])
        # phase 2, whatever it retries, binds inside the total computed at submit
        for nr in sorted(r for r in {0, 1, 2, ns // 2, ns - 1, ns} if 0 <= r <= ns):
            R, _, _ = sm_layout(lib, nj, ns, rows, by_index, agg, nr=nr)
            assert {k: v for k, v in R.items() if k not in dict(phase2) and k != "pipe2"} == \
                   {k: v for k, v in L.items() if k not in dict(phase2) and k != "pipe2"}
            assert R["pipe2"] == check_run([(n, R[n], z) for n, z in sm_sizes(nj, ns, rows, by_index, nr)[3]], late)
            assert late <= R["d_rset"] and R["pipe2"] <= L["pipe2"] and R["pipe2"] + p2 <= L["ws_end"]
        totals[nj, ns] = (L["ws_end"], L["pin_end"])
    for nj, (a, b) in itertools.product(JOBS, zip(SETS, SETS[1:])):
        assert totals[nj, a][0] <= totals[nj, b][0] and totals[nj, a][1] <= totals[nj, b][1], (nj, a, b)
    for ns, (a, b) in itertools.product(SETS, zip(JOBS, JOBS[1:])):
        assert totals[a, ns][0] <= totals[b, ns][0] and totals[a, ns][1] <= totals[b, ns][1], (ns, a, b)


def test_same_message_front_alone(lib):
    """lb_same_message_aggregates: the front's buffers and the decode records, nothing of the rest."""
    for nj, ns in itertools.product(JOBS, SETS):
        L, _, _ = sm_layout(lib, nj, ns, 0, 0, 0, front_only=True)
        inputs, phase1, dec, phase2, pinned = sm_sizes(nj, ns, 0, 0, ns)
        assert all(L[n] < 0 for n, _ in phase2 + phase1[7:] + pinned[4:])
        front_end = check_run([(n, L[n], z) for n, z in phase1[:7]], L["in_bytes"])
        assert L["pipe1"] == front_end
        assert L["ws_end"] == check_run([(n, L[n], z) for n, z in dec], front_end)
        assert L["pin_end"] == check_run([(n, L[n], z) for n, z in pinned[:4]], L["in_bytes"])


# ---- the host-buffer call and the latency path ---------------------------------------------------
def test_host_call_layout(lib):
    names = "req pko pk msg sigo sig seed rows valid err sst".split()
    for nr, ns, keys, rows, pk_off, by_index in [(0, 0, 1, 0, 0, 0), (1, 1, 1, 0, 0, 0), (3, 130, 1, 0, 0, 1),
                                                 (3, 130, 1, 5, 0, 1), (512, 65536, 1, 0, 0, 0), (8, 1024, 16, 0, 1, 0)]:
        n_pk = ns * keys
        off = (LL * (len(names) + 1))()
        end = lib.cv_host_layout(nr, ns, n_pk, 96 * ns, rows, pk_off, by_index, off)
        L = dict(zip(names, off))
        sizes = [("req", 4 * (nr + 1)), ("pko", 4 * (ns + 1)), ("pk", n_pk * (4 if by_index else 96)), ("msg", 32 * ns),
                 ("sigo", 4 * (ns + 1)), ("sig", 96 * ns), ("seed", 32), ("rows", 96 * rows)]
        assert (L["pko"] >= 0) == bool(pk_off) and (L["rows"] >= 0) == bool(rows)
        in_bytes = al(check_run([(n, L[n], z) for n, z in sizes]))
        assert off[len(names)] == in_bytes
        outs = [("valid", max(nr, 1)), ("err", max(nr, 1)), ("sst", max(ns, 1))]
        assert end == check_run([(n, L[n], z) for n, z in outs], in_bytes)
        # (finish_slot's pinned rows: the two request rows one aligned row apart)
        assert L["err"] - L["valid"] == L["sst"] - L["err"] == al(max(nr, 1))


@pytest.mark.parametrize("ns", [1, 2, 896])
def test_lp_ws_bytes_is_the_end_of_run_lps_list(lib, ns):
    sizes = [144 * ns, ns, 4 * ns * 11 * 16, 4 * ns * 67, ns, 4 * ns, 4 * ns * 12 * 16, 4 * 20 * ns, 32]
    for own in (1, 0):
        off = (LL * 9)()
        end = lib.cv_lp_layout(ns, own, 0, off)
        bufs = [(str(i), off[i], z) for i, z in enumerate(sizes)]
        assert (off[4] >= 0) == bool(own)
        assert end == check_run(bufs)
        if own:
            assert lib.cv_lp_ws_bytes(ns) == end
        else:  # the caller's status buffer in place of the call's own: never more than the bound
            assert end <= lib.cv_lp_ws_bytes(ns)
    off = (LL * 9)()
    assert lib.cv_lp_layout(ns, 1, 7, off) == lib.cv_lp_ws_bytes(ns) + 256 and off[0] == 256


# ---- the capacity of a context-owned device array ------------------------------------------------
TABLE, LIST = (4096, 1), (1024, 0)  # (floor, doubling): the pubkey and balance tables; the index lists


def test_device_array_capacity(lib):
    cap = lambda have, need, policy: lib.cv_dev_array_cap(have, need, *policy)  # noqa: E731
    top = lib.cv_dev_array_max()
    assert top == 2 ** 31 - 1
    # the first reservation, below and above the floor
    assert cap(0, 1, TABLE) == 4096 and cap(0, 5000, TABLE) == 5000
    assert cap(0, 1, LIST) == 1024 and cap(0, 1025, LIST) == 1025
    # it fits: no move; one more: a table doubles, a list takes exactly the need
    assert cap(4096, 4096, TABLE) == 4096 and cap(4096, 4097, TABLE) == 8192
    assert cap(8192, 20000, TABLE) == 20000  # (more than the double)
    assert cap(1024, 1024, LIST) == 1024 and cap(1024, 1025, LIST) == 1025 and cap(5000, 5001, LIST) == 5001
    assert cap(5000, 3, LIST) == 5000  # (a list never shrinks)
    # a doubling past the table's limit stops at it
    assert cap(2 ** 30 + 5, 2 ** 30 + 6, TABLE) == top and cap(top - 1, top, TABLE) == top
    rng = random.Random(7)
    for _ in range(2000):
        have = rng.choice((0, 1, 1024, 4096, rng.randrange(2 ** 31), rng.randrange(2 ** 20)))
        need = rng.choice((0, 1, have, min(have + 1, top), rng.randrange(2 ** 31), rng.randrange(2 ** 20)))
        for policy in (TABLE, LIST):
            got = cap(have, need, policy)
            assert got >= need and (got == have if need <= have else got >= policy[0])
            if need > have:
                assert got <= top and (got == max(need, policy[0]) if policy is LIST else
                                       got == min(max(2 * have, need, 4096), top))


def test_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "carve_host_main")
    base = ["g++", "-O1", "-std=c++17", "-DCARVE_HOST_MAIN", "-o", exe, SRC]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                         capture_output=True)
    if san.returncode != 0:  # no sanitizer runtime with this compiler: the plain program still walks the grid
        subprocess.check_call(base)
    res = subprocess.run([exe, str(DEC_MAX)], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.stdout, res.stderr)
