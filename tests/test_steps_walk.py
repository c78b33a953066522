"""The lane walk of the step-major accumulation (lodestar_amd/csrc/bls_steps_walk.h) on the host: a
g++ build of the header behind ctypes (tests/native/steps_walk_host.cpp), against a Python
restatement of the loop step_lines ran before the walk was a function of its own.  k_step_acc and
k_line_pairs both enumerate a lane's items with this code, so what is checked here is that the
pairs one kernel multiplies are the pairs the other reads.  Also the plan's pair_pre rule at its
size threshold (bls_plan.h).  A stand-alone build of the same file walks everything under
-fsanitize=address,undefined where the host compiler has the runtime."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "steps_walk_host.cpp")
LINES = 68
SPLITS = (1, 2, 4)  # lanes per set: 68, 34, 17 lines per lane


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("steps_walk") / "libsteps_walk_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC])
    L = ctypes.CDLL(out)
    L.sw_items.argtypes = [ctypes.c_uint] * 3 + [ctypes.c_int, ctypes.POINTER(ctypes.c_uint)]
    L.sw_pair_at.argtypes = [ctypes.c_uint] * 4 + [ctypes.POINTER(ctypes.c_uint)]
    L.sw_env_set.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    L.sw_plan.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.sw_pair_pre_min_sets.restype = ctypes.c_uint
    return L


def items(lib, n, t0, L, pairs=True):
    buf = (ctypes.c_uint * (3 * L))()
    k = lib.sw_items(n, t0, L, int(pairs), buf)
    return [(buf[3 * e], buf[3 * e + 1], bool(buf[3 * e + 2])) for e in range(k)]


def step_lines_order(n, t0, cnt, paired=True):
    """step_lines' loop as it stood (k_steps.hip): (j, i, two lines at once) per iteration"""
    j, i = divmod(t0, n)
    out, c = [], 0
    while c < cnt:
        if paired and i + 1 < n and c + 1 < cnt:
            out.append((j, i, True))
            i += 2
            c += 2
        else:
            out.append((j, i, False))
            i += 1
            c += 1
        if i >= n:
            i -= n
            j += 1
    return out


@pytest.mark.parametrize("split", SPLITS)
def test_walk_every_request_size(lib, split):
    L = LINES // split
    ji = (ctypes.c_uint * 2)()
    for n in range(1, 131):
        seen = [0] * (LINES * n)
        for lane in range(n * split):
            t0 = LINES * (lane // split) + L * (lane % split)
            got = items(lib, n, t0, L)
            assert got == step_lines_order(n, t0, L), (n, lane)  # today's order, item by item
            pairs = [(j, i) for j, i, two in got if two]
            assert len(pairs) <= L // 2 and len(pairs) <= 34, (n, lane)
            for j, i, two in got:
                assert j < LINES and i + two < n, (n, lane)  # a pair's two lines share step j
                for d in range(1 + two):
                    seen[j * n + i + d] += 1
            # the u-th pair, as k_line_pairs' thread u finds it; none past the lane's count
            for u, (j, i) in enumerate(pairs):
                assert lib.sw_pair_at(n, t0, L, u, ji) == 1 and (ji[0], ji[1]) == (j, i), (n, lane, u)
            assert lib.sw_pair_at(n, t0, L, len(pairs), ji) == 0 and lib.sw_pair_at(n, t0, L, 34, ji) == 0, (n, lane)
            # one line at a time (k_step_acc MODE 2)
            assert items(lib, n, t0, L, pairs=False) == step_lines_order(n, t0, L, paired=False), (n, lane)
        assert seen == [1] * (LINES * n), n  # every line t in [0, 68 n): exactly once


def test_pair_counts_by_hand(lib):
    # a 1-set request has no pairs; a 2-set request one per step; 3 sets: pair + single per step,
    # a lane's 68 lines being 22 steps and two more lines (a pair when they start a step)
    assert [two for _, _, two in items(lib, 1, 0, 68)] == [False] * 68
    assert items(lib, 2, 68, 68) == [(34 + s, 0, True) for s in range(34)]
    got = items(lib, 3, 0, 68)
    assert got[:3] == [(0, 0, True), (0, 2, False), (1, 0, True)] and got[-1] == (22, 0, True) and len(got) == 45
    # a lane that starts on a step's last line and ends on a step's first
    assert items(lib, 69, 68, 68)[0] == (0, 68, False) and items(lib, 69, 68, 68)[-1] == (1, 66, False)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pair_pre_threshold(lib, mode):
    assert lib.sw_pair_pre_compiled() == 1 and lib.sw_pair_pre_min_sets() == 8192
    lib.sw_env_clear()
    lib.sw_env_set(b"LB_STEP_MODE", str(mode).encode())
    for lone in (0, 1):
        for sets, above in ((8191, False), (8192, True)):
            assert lib.sw_plan(64, sets, lone, 0, 1) == mode and lib.sw_plan(64, sets, lone, 0, 3) == 1
            assert lib.sw_plan(64, sets, lone, 0, 2) == lib.sw_lines_rows()
            assert bool(lib.sw_plan(64, sets, lone, 0, 0)) == (above and mode != 2), (mode, lone, sets)
        assert lib.sw_plan(512, 65536, lone, 0, 0) == (mode != 2)
        assert lib.sw_plan(512, 65536, lone, 1, 0) == (mode != 2)  # (a two-phase call too)
    lib.sw_env_clear()
    # the round-program lines band and everything below the threshold keep their launches
    assert not any(lib.sw_plan(8, n, lone, 0, 0) for n in (1025, 4704, 5120, 5121, 8191) for lone in (0, 1))
    # the pairs organisation has no lanes to walk
    lib.sw_env_set(b"LB_ACC", b"pairs")
    assert lib.sw_plan(64, 65536, 0, 0, 0) == 0
    lib.sw_env_clear()


def test_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "steps_walk_host_main")
    base = ["g++", "-O1", "-std=c++17", "-DSTEPS_WALK_HOST_MAIN", "-o", exe, SRC]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                         capture_output=True)
    if san.returncode != 0:  # no sanitizer runtime with this compiler: the plain program still walks everything
        subprocess.check_call(base)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.stdout, res.stderr)
