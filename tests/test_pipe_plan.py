"""Planning of a pipeline call (lodestar_amd/csrc/bls_plan.h) on the host: a g++ build of the
header behind ctypes (tests/native/plan_host.cpp).  The plans against DESIGN.md §4.5's rules,
written out by hand here; the environment table switch by switch, quirks included; and the
workspace layout over a grid of shapes and configs: aligned, disjoint, complete, bounded by
plan_upper's, and plan_upper's monotone.  A stand-alone build of the same file walks the grid
under -fsanitize=address,undefined where the host compiler has the runtime."""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "plan_host.cpp")

HASH_NONE, HASH_PLAIN, HASH_FINISH_LP, HASH_FULL_LP = range(4)
LINES_NONE, LINES_PLAIN, LINES_ROWS, LINES_LP = range(4)
DECODE_NONE, DECODE_PLAIN, DECODE_LP = range(3)


class Lib:
    def __init__(self, path):
        L = self.L = ctypes.CDLL(path)
        L.pp_config_new.restype = ctypes.c_void_p
        L.pp_config_free.argtypes = [ctypes.c_void_p]
        L.pp_config_get.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        L.pp_config_get.restype = ctypes.c_longlong
        L.pp_config_field.restype = ctypes.c_char_p
        L.pp_env_knob.restype = ctypes.c_char_p
        L.pp_env_set.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        L.pp_plan_new.restype = ctypes.c_void_p
        L.pp_plan_new.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint] + [ctypes.c_int] * 4
        L.pp_plan_upper_new.restype = ctypes.c_void_p
        L.pp_plan_upper_new.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint]
        L.pp_plan_free.argtypes = [ctypes.c_void_p]
        L.pp_plan_get.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
        L.pp_plan_get.restype = ctypes.c_longlong
        L.pp_buf_name.restype = ctypes.c_char_p
        L.pp_layout.restype = ctypes.c_ulonglong
        L.pp_layout.argtypes = [ctypes.c_void_p, ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_void_p]
        L.pp_upper_bytes.restype = ctypes.c_ulonglong
        L.pp_upper_bytes.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_uint]
        L.pp_lp_ws_bytes.restype = ctypes.c_ulonglong
        L.pp_lp_ws_bytes.argtypes = [ctypes.c_ulonglong]
        self.bufs = [L.pp_buf_name(i).decode() for i in range(L.pp_buf_count())]
        self.cfg_fields = [L.pp_config_field(i).decode() for i in range(L.pp_config_nfields())]
        self.knobs = [L.pp_env_knob(i).decode() for i in range(L.pp_env_nknobs())]

    def config(self, env=None):
        """A PipeConfig from the defaults and `env` (through config_from_env's lookup callback)."""
        self.L.pp_env_clear()
        for k, v in (env or {}).items():
            self.L.pp_env_set(k.encode(), v.encode())
        return self.L.pp_config_new(1)

    def config_dict(self, env=None):
        c = self.config(env)
        try:
            return {f: self.L.pp_config_get(c, f.encode()) for f in self.cfg_fields}
        finally:
            self.L.pp_config_free(c)

    def plan(self, n_req, n_sets, lone=False, partial=False, presigned=False, prio=False, env=None, upper=False,
             start=0):
        """-> (plan fields, {buffer: (offset, bytes)} of the present buffers in order, total bytes)"""
        c = self.config(env)
        p = self.L.pp_plan_upper_new(c, n_req, n_sets) if upper else self.L.pp_plan_new(
            c, n_req, n_sets, int(lone), int(partial), int(presigned), int(prio))
        try:
            names = ("n_req n_sets ns nr1 lone partial presigned latency_path lone_mid by_lines by_wave f_sets lines_buf "
                     "tail_wave merged n_pairs use_msm steps split fold mtail mt_wide msm_wide bits_lp rtail n_ent "
                     "max_chunks msm_short msm_T lsplit dec_lp hf_lp hash_full hf_narrow lines_lp dec_sets hf_sets "
                     "ll_sets level_wc lvl_per needs_lp tp_release mt_out fx halves hash lines decode miller_wave "
                     "miller_sets lines_W step_M step_W acc_lpr").split()
            f = {n: self.L.pp_plan_get(p, n.encode()) for n in names}
            assert -999 not in f.values()
            off = (ctypes.c_longlong * len(self.bufs))()
            size = (ctypes.c_ulonglong * len(self.bufs))()
            total = self.L.pp_layout(p, start, off, size)
            lay = {b: (off[i], size[i]) for i, b in enumerate(self.bufs) if off[i] >= 0}
            return f, lay, total
        finally:
            self.L.pp_plan_free(p)
            self.L.pp_config_free(c)

    def upper_bytes(self, n_req, n_sets, env=None):
        c = self.config(env)
        try:
            return self.L.pp_upper_bytes(c, n_req, n_sets)
        finally:
            self.L.pp_config_free(c)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plan") / "libplan_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC])
    return Lib(out)


def check(f, **want):
    got = {k: (bool(f[k]) if isinstance(v, bool) else f[k]) for k, v in want.items()}
    assert got == want


# ---- 1. the plans against DESIGN §4.5's rules ---------------------------------------------
def test_c2_shared_and_lone(lib):
    f, _, _ = lib.plan(512, 65536)
    check(f, latency_path=False, steps=True, use_msm=True, merged=True, mtail=True, mt_wide=False, msm_wide=False,
          bits_lp=False, lsplit=1, msm_T=16, dec_lp=False, hf_lp=False, lines_lp=False, level_wc=True, rtail=True,
          hash=HASH_PLAIN, lines=LINES_ROWS, decode=DECODE_PLAIN, lines_W=2, step_M=1, step_W=1, needs_lp=True)
    f, _, _ = lib.plan(512, 65536, lone=True)
    check(f, mt_wide=True, msm_wide=True, bits_lp=True, lsplit=1, msm_T=16, steps=True, mtail=True)


def test_lone_c5(lib):
    f, _, _ = lib.plan(32, 4704, lone=True)
    check(f, lsplit=4, dec_lp=True, lines_lp=True, hf_lp=False, msm_T=4, msm_short=True, lines=LINES_LP,
          decode=DECODE_LP, hash=HASH_PLAIN)


def test_lone_hash_thresholds(lib):
    check(lib.plan(32, 1536, lone=True)[0], hf_lp=True, hash_full=True, hash=HASH_FULL_LP)
    check(lib.plan(32, 2048, lone=True)[0], hf_lp=True, hash_full=True)
    for n in (2049, 3072):
        check(lib.plan(32, n, lone=True)[0], hf_lp=True, hash_full=False, hash=HASH_FINISH_LP, hf_narrow=True)
    check(lib.plan(32, 3073, lone=True)[0], hf_lp=False, hash_full=False, hash=HASH_PLAIN)
    check(lib.plan(32, 1536)[0], hf_lp=False, hash=HASH_PLAIN)  # (not lone: none of the programs)


def test_lone_decode_lines_thresholds(lib):
    check(lib.plan(32, 5120, lone=True)[0], dec_lp=True, lines_lp=True, decode=DECODE_LP, lines=LINES_LP)
    check(lib.plan(32, 5121, lone=True)[0], dec_lp=False, lines_lp=False, decode=DECODE_PLAIN, lines=LINES_ROWS)


def test_lone_split_thresholds(lib):
    check(lib.plan(32, 16384, lone=True)[0], lsplit=4, msm_short=True, msm_T=4)
    check(lib.plan(32, 16385, lone=True)[0], lsplit=2, msm_short=False, msm_T=16)
    check(lib.plan(32, 32768, lone=True)[0], lsplit=2)
    check(lib.plan(32, 32769, lone=True)[0], lsplit=1)
    check(lib.plan(32, 16384)[0], lsplit=1, msm_short=False, msm_T=16)


def test_latency_path_rules(lib):
    check(lib.plan(1, 896, lone=True)[0], latency_path=True)
    for n in (897, 1024):
        check(lib.plan(1, n, lone=True)[0], latency_path=False, lone_mid=True, merged=True, steps=True, use_msm=True,
              mtail=True, by_lines=True)
    check(lib.plan(1, 1024)[0], latency_path=True)
    check(lib.plan(1, 1024, lone=True, prio=True)[0], latency_path=True, lone_mid=False)
    check(lib.plan(1, 1024, lone=True, env={"LB_LP_MAX": "1024"})[0], latency_path=True, lone_mid=False)
    check(lib.plan(7, 1025)[0], latency_path=False, merged=False, use_msm=False, steps=True, rtail=False)
    check(lib.plan(8, 1025)[0], latency_path=False, merged=True, use_msm=True)


def test_partial_and_presigned(lib):
    for env in ({}, {"LB_TAIL": "lane"}):
        check(lib.plan(1, 10, partial=True, env=env)[0], latency_path=False, merged=True, tail_wave=True,
              by_wave=True, miller_wave=True, use_msm=False)
    f, lay, _ = lib.plan(10, 10, presigned=True)
    check(f, latency_path=False, decode=DECODE_NONE, dec_lp=False)
    assert "sig" not in lay and "rsig" in lay
    check(lib.plan(10, 10, presigned=True, lone=True)[0], decode=DECODE_NONE, dec_lp=False, dec_sets=0)


def test_pairs_organisation(lib):
    check(lib.plan(64, 8192, lone=True, env={"LB_ACC": "pairs"})[0], steps=False, split=True, fold=False,
          use_msm=True, halves=True, fx=False, lines=LINES_PLAIN)
    check(lib.plan(63, 8192, lone=True, env={"LB_ACC": "pairs"})[0], split=False, fold=True)
    check(lib.plan(512, 65536, env={"LB_ACC": "pairs"})[0], steps=False, split=False, fold=True, use_msm=True, fx=True,
          mtail=False, level_wc=False, acc_lpr=64)


def test_mtail_off(lib):
    # (the one-wave chain: msm_final + lines of S_all + horner_all + k_tail, and k_msm_bits' threads)
    check(lib.plan(512, 65536, lone=True, env={"LB_MTAIL": "0"})[0], mtail=False, bits_lp=False, use_msm=True,
          steps=True, fold=False, msm_wide=True, mt_out=False)


def test_lane_tails(lib):
    f, lay, _ = lib.plan(16, 2000, env={"LB_TAIL": "lane", "LB_MILLER": "lane"})
    check(f, tail_wave=False, lines_buf=False, merged=False, steps=False, miller_sets=True, lines=LINES_NONE)
    assert "lines" not in lay and "f_sets" in lay
    f, lay, _ = lib.plan(16, 2000, env={"LB_TAIL": "lane"})
    check(f, tail_wave=False, by_lines=True, lines_buf=True, merged=False, steps=False, rtail=False)
    assert "lines" in lay
    check(lib.plan(16, 2000, partial=True, env={"LB_TAIL": "lane"})[0], merged=True, tail_wave=True)


def test_forced_step_split(lib):
    check(lib.plan(512, 65536, env={"LB_STEP_SPLIT": "4"})[0], lsplit=4)
    check(lib.plan(512, 65536, lone=True, env={"LB_STEP_SPLIT": "2"})[0], lsplit=2)


def test_no_sets(lib):
    # (an empty call is the latency path's whatever its bound, 0 <= 0; a two-phase one the pipeline's)
    check(lib.plan(3, 0, env={"LB_LP_MAX": "0"})[0], latency_path=True)
    f, lay, _ = lib.plan(3, 0, partial=True)
    check(f, latency_path=False, ns=1, merged=True, n_pairs=4, hash=HASH_NONE, lines=LINES_NONE, decode=DECODE_NONE, steps=False,
          use_msm=False, miller_wave=False, miller_sets=False, dec_lp=False, hf_lp=False, lines_lp=False)
    assert lay["sig"][1] == 288 and lay["pk"][1] == 144 and lay["q"][1] == 576 and lay["single"][1] == 1
    check(lib.plan(3, 0, lone=True, partial=True)[0], dec_lp=False, hf_lp=False, steps=False, hash=HASH_NONE)


# ---- 2. the environment table ----------------------------------------------------------------
DEFAULTS = dict(miller_mode=0, lines_min_sets=1025, wave_max_sets=1024, lines_waves=2, lines_waves_small=1, acc_lpr=64,
                acc_split=-1, acc_steps=1, step_mode=1, step_waves=1, tail_wave=1, merge_min_req=8, msm_min_sets=1025,
                level_wc=1, msm_lanes=1, wide_tail=1, msm_bits_lp=1, step_split=0, lp_decode=1, lp_hash_finish=1,
                msm_short=1, msm_short_max=16384, msm_t_lone=4, lp_dec_max=5120, lp_hf_max=3072, lp_lines_max=5120,
                lp_hash_full=2048, lp_narrow=1, lp_lines=1, lp_max_sets=1024, lp_lone_max=896, lp_explicit=0,
                mtail_lp=1, rtail_lp=1, tp_release=1, tp_release_cfg=1)

_FLAGS = {"LB_LEVEL": "level_wc", "LB_MSM_LANES": "msm_lanes", "LB_WIDE_TAIL": "wide_tail",
          "LB_MSM_BITS_LP": "msm_bits_lp", "LB_LP_DECODE": "lp_decode", "LB_LP_HASH_FINISH": "lp_hash_finish",
          "LB_LP_LINES": "lp_lines", "LB_MSM_SHORT": "msm_short", "LB_MTAIL": "mtail_lp", "LB_RTAIL": "rtail_lp"}
_NUMBERS = {"LB_MERGE_MIN": "merge_min_req", "LB_MSM_MIN": "msm_min_sets", "LB_LINES_MIN": "lines_min_sets",
            "LB_WAVE_MAX": "wave_max_sets", "LB_LP_HASH_FULL": "lp_hash_full", "LB_LP_NARROW": "lp_narrow",
            "LB_LP_DEC_MAX": "lp_dec_max", "LB_LP_HF_MAX": "lp_hf_max", "LB_LP_LINES_MAX": "lp_lines_max",
            "LB_MSM_SHORT_MAX": "msm_short_max", "LB_LP_LONE_MAX": "lp_lone_max"}
# switch -> [(value, the fields it changes from the defaults)]
ENV_CASES = {
    "LB_MILLER": [("lane", dict(miller_mode=1)), ("lines", dict(miller_mode=2)), ("wave", dict(miller_mode=3)),
                  ("auto", {}), ("2", {})],
    "LB_TAIL": [("lane", dict(tail_wave=0)), ("wave", {}), ("0", {})],
    "LB_ACC": [("pairs", dict(acc_steps=0)), ("steps", {}), ("0", {})],
    "LB_ACC_SPLIT": [("1", dict(acc_split=1)), ("0", dict(acc_split=0)), ("-1", dict(acc_split=1))],
    "LB_ACC_LPR": [("32", dict(acc_lpr=32)), ("16", dict(acc_lpr=16)), ("64", {}), ("8", {})],
    "LB_LINES_WAVES": [("1", dict(lines_waves=1, lines_waves_small=1)), ("2", dict(lines_waves_small=2)),
                       ("3", dict(lines_waves_small=2))],
    "LB_STEP_MODE": [("0", dict(step_mode=0)), ("2", dict(step_mode=2)), ("7", dict(step_mode=7))],
    "LB_STEP_WAVES": [("2", dict(step_waves=2)), ("1", {}), ("3", {})],
    "LB_STEP_SPLIT": [("1", dict(step_split=1)), ("2", dict(step_split=2)), ("4", dict(step_split=4)), ("3", {}),
                      ("8", {})],
    "LB_MSM_T_LONE": [("1", dict(msm_t_lone=1)), ("16", dict(msm_t_lone=16)), ("0", {}), ("17", {})],
    "LB_LP_MAX": [("0", dict(lp_max_sets=0, lp_explicit=1)), ("-5", dict(lp_max_sets=0, lp_explicit=1)),
                  ("512", dict(lp_max_sets=512, lp_explicit=1)), ("1024", dict(lp_explicit=1)),
                  ("99999999", dict(lp_max_sets=1 << 20, lp_explicit=1))],
    "LB_TP_RELEASE": [("0", dict(tp_release=0, tp_release_cfg=0)), ("1", {})],
}
for _k, _f in _FLAGS.items():
    ENV_CASES[_k] = [("0", {_f: 0}), ("1", {}), ("2", {})]
for _k, _f in _NUMBERS.items():
    ENV_CASES[_k] = [("0", {_f: 0}), ("7", {_f: 7}), ("70000", {_f: 70000})]


def test_env_defaults(lib):
    assert lib.config_dict() == DEFAULTS
    assert sorted(lib.knobs) == sorted(ENV_CASES)  # every switch of the table has its cases here


@pytest.mark.parametrize("name", sorted(ENV_CASES))
def test_env_switch(lib, name):
    for value, changed in ENV_CASES[name]:
        assert lib.config_dict({name: value}) == dict(DEFAULTS, **changed), (name, value)


# ---- 3. the layout -----------------------------------------------------------------------------
SETS = [0, 1, 2, 67, 68, 69, 1025, 4704, 65536, 1048576]
CONFIGS = [{}, {"LB_ACC": "pairs"}, {"LB_ACC": "pairs", "LB_ACC_SPLIT": "1"}, {"LB_TAIL": "lane"}, {"LB_MTAIL": "0"},
           {"LB_LEVEL": "0"}, {"LB_STEP_SPLIT": "4"}, {"LB_MSM_T_LONE": "1"}]
SZ = dict(g2j=288, g1j=144, g2a=192, fp12=576)


def _required(f):
    """The buffers a plan's flags require (besides the unconditional ones)."""
    need = {"rsig", "q", "h", "pk", "rpk", "single", "pk_st", "sig_st", "S", "fS", "F", "bad", "Sall", "Fall", "mflag", "mstats"}
    if not f["presigned"]:
        need.add("sig")
    if not f["by_lines"]:
        need.add("f_sets")
    if f["by_lines"] or f["by_wave"] or f["tail_wave"]:
        need.add("lines")
    if f["rtail"]:
        need |= {"rt_in", "rt_fl"}
    if f["use_msm"]:
        need |= {"mkeys", "msorted", "mhist", "mcsum", "mbsum", "mG"}
    if f["steps"]:
        need |= {"rhist", "rgt", "rowoff", "rpos", "rinv", "rmeta", "G", "Pl"}
        if f["lsplit"] > 1:
            need.add("Fparts")
    if f["dec_lp"]:
        need |= {"dec_in", "dec_fl", "dec_out", "dec_ofl", "dec_pre"}
    if f["hf_lp"]:
        need |= {"hf_in", "hf_out"}
    if f["lines_lp"]:
        need |= {"ll_in", "ll_out"}
    if f["level_wc"]:
        need |= {"lvA", "lvB", "lhA", "lhB"}
    if f["mtail"]:
        need.add("mt_in")
        if f["partial"]:
            need.add("mt_out")
    if f["bits_lp"]:
        need |= {"mb_in0", "mb_in1", "mb_in2"}
    if f["fold"]:
        need.add("Fx")
    if f["split"]:
        need |= {"off2", "acc_F", "acc_bad", "acc_err"}
    if f["partial"]:
        need.add("partial")
    return need


def _check_layout(lib, f, lay, total, n_req, n_sets):
    end = 0
    for name, (off, size) in lay.items():  # (in layout order)
        assert off % 256 == 0 and off >= end and size > 0, (name, off, size, end)
        end = off + size
    assert total == end
    assert set(lay) == _required(f), (set(lay) ^ _required(f))
    ns = max(n_sets, 1)
    n_pairs = n_sets + n_req + (1 if f["merged"] else 0)
    if "lines" in lay:
        assert lay["lines"][1] == n_pairs * 68 * 72 * 4
    if f["steps"]:
        assert lay["G"][1] == 144 * 4 * ns * f["lsplit"]
    if f["use_msm"]:
        assert lay["mkeys"][1] == lay["msorted"][1] == 4 * 2 * 3 * n_sets
        assert lay["mcsum"][1] == SZ["g2j"] * (2 * 3 * n_sets // f["msm_T"] + 3 * 1024)
    if f["level_wc"]:
        assert f["lvl_per"] % 256 == 0 and 256 <= f["lvl_per"] <= 2048
        assert lay["lvA"][1] == SZ["fp12"] * 63 * f["lvl_per"]
        assert lay["lvB"][1] == SZ["fp12"] * 63 * ((f["lvl_per"] + 7) // 8)


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_layout_grid(lib, ci):
    env = dict(CONFIGS[ci], LB_LP_MAX="0")  # (the pipeline's own layout at every size)
    for n in SETS:
        for r in sorted({1, 8, max(n // 128, 1), max(n, 1)}):
            upper = lib.upper_bytes(r, n, env)
            for lone, partial, presigned in itertools.product((False, True), repeat=3):
                f, lay, total = lib.plan(r, n, lone, partial, presigned, env=env)
                assert total <= upper, (n, r, lone, partial, presigned)
                if f["latency_path"]:  # (only the empty one-phase call: 0 sets <= a bound of 0)
                    assert n == 0 and not partial and not presigned and not lay
                    continue
                _check_layout(lib, f, lay, total, r, n)
                # from an unaligned fill of the slab: the same buffers, one alignment step later at most
                _, lay7, total7 = lib.plan(r, n, lone, partial, presigned, env=env, start=7)
                assert all(o % 256 == 0 for o, _ in lay7.values()) and total7 <= total + 255


def test_latency_path_calls_fit_the_upper_bound(lib):
    for n in (0, 1, 2, 67, 128, 896, 1024):
        for r in sorted({1, max(n // 128, 1), max(n, 1)}):
            for lone in (False, True):
                f, lay, total = lib.plan(r, n, lone)
                if f["latency_path"]:
                    assert not lay and total == lib.L.pp_lp_ws_bytes(max(n, 1))
                assert total <= lib.upper_bytes(r, n)
    # run_lp's nine buffers, by hand: 1,024 sets
    ns, want = 1024, 0
    for z in (144 * ns, ns, 4 * ns * 11 * 16, 4 * ns * 67, ns, 4 * ns, 4 * ns * 12 * 16, 4 * 20 * ns, 32):
        want = (want + 255) // 256 * 256 + z
    assert lib.L.pp_lp_ws_bytes(ns) == want


def test_upper_layout_holds_every_buffer(lib):
    f, lay, total = lib.plan(8, 0, upper=True)
    assert list(lay) == lib.bufs and lay["mkeys"][1] == lay["msorted"][1] == 0  # (no sets: no MSM entries)
    assert all(size > 0 for name, (_, size) in lay.items() if name not in ("mkeys", "msorted"))
    f, lay, total = lib.plan(512, 65536, upper=True)
    assert list(lay) == lib.bufs and f["lsplit"] == 4 and f["msm_T"] == 4


@pytest.mark.parametrize("ci", range(len(CONFIGS)))
def test_upper_monotone(lib, ci):
    env = CONFIGS[ci]
    c = lib.config(env)
    try:
        up = lambda r, n: lib.L.pp_upper_bytes(c, r, n)  # noqa: E731
        prev = 0
        for n in range(0, 6001):
            u = up(47, n)
            assert u >= prev, n
            prev = u
        edges = sorted({t + d for t in (896, 1024, 1025, 2048, 3072, 5120, 16384, 32768, 65536, 1 << 20)
                        for d in (-1, 0, 1)})
        for a, b in zip(edges, edges[1:]):
            assert up(512, a) <= up(512, b) and up(a, 1 << 20) <= up(b, 1 << 20), (a, b)
        for r in range(0, 600):
            assert up(r, 4704) <= up(r + 1, 4704), r
    finally:
        lib.L.pp_config_free(c)


def test_no_32bit_wrap(lib):
    n, r = 1 << 20, 8192
    f, lay, total = lib.plan(r, n, lone=True, env={"LB_STEP_SPLIT": "4"})
    assert f["lsplit"] == 4 and f["steps"] and f["use_msm"]
    assert lay["G"][1] == 144 * 4 * n * 4 > 1 << 31
    assert lay["lines"][1] == (n + r + 1) * 68 * 72 * 4 > 1 << 34
    assert lay["mkeys"][1] == 4 * 6 * n and f["n_ent"] == 6 * n
    assert total > lay["lines"][1] + lay["G"][1] and total <= lib.upper_bytes(r, n, {"LB_STEP_SPLIT": "4"})


def test_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "plan_host_main")
    base = ["g++", "-O1", "-std=c++17", "-DPLAN_HOST_MAIN", "-o", exe, SRC]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
                         capture_output=True)
    if san.returncode != 0:  # no sanitizer runtime with this compiler: the plain program still walks the grid
        subprocess.check_call(base)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and res.stdout.strip() == "ok", (res.stdout, res.stderr)
