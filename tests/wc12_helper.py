"""The generated wave-cooperative Fp12 programs (lodestar_amd/csrc/gen_wc12.py) as Python
objects, and their evaluation modulo p: shared by tests/test_wc12_programs.py (CPU, against
the oracle), tests/pairing_cases.py (the extreme operand patterns) and
tests/test_gpu_pairing.py (the expectation for every program, LB_WC_CYC on non-cyclotomic
inputs included)."""
import functools
import importlib.util
import os

from oracle import bls12_381 as O

P = O.P
_spec = importlib.util.spec_from_file_location(
    "gen_wc12", os.path.join(os.path.dirname(__file__), "..", "lodestar_amd", "csrc", "gen_wc12.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)

# program names in table order (LB_WC_<name> = index)
NAMES = [name for name, _ in G.OPS]
INDEX = {name: i for i, name in enumerate(NAMES)}


@functools.lru_cache(maxsize=None)
def program(name):
    """(Program, [12 output forms]) of LB_WC_<name>."""
    prog, out = dict(G.OPS)[name]()
    return prog, out.flat()


def flat(f12):
    out = []
    for f6 in f12:
        for f2 in f6:
            out += [f2[0], f2[1]]
    return out


def unflat(v):
    f2 = [(v[2 * k], v[2 * k + 1]) for k in range(6)]
    return ((f2[0], f2[1], f2[2]), (f2[3], f2[4], f2[5]))


def evaluate(prog, outs, A, B):
    """The program on coefficient lists A, B (B is A for a square program's caller)."""
    env = {}

    def ev(form):
        acc = 0
        for (kind, i), c in form.d.items():
            v = A[i] if kind == "A" else B[i] if kind == "B" else env[i]
            acc += c * v
        return acc % P

    for k, (x, y) in enumerate(prog.prods):
        env[k] = ev(x) * ev(y) % P
    return [ev(o) for o in outs]


def run(prog_fn, A, B):
    prog, out = prog_fn()
    return evaluate(prog, out.flat(), A, B)


def run_named(name, A, B):
    prog, outs = program(name)
    return evaluate(prog, outs, A, B)
