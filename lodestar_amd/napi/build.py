"""Build the N-API addon (addon.cc -> lodestar_bls.node) against the node
headers in /usr/include/node (N-API is ABI-stable: the same addon loads in any
node >= 12.22 that offers N-API 8, including the node 20 line the reference
requires).  Links liblodestar_bls.so from the package directory (rpath
$ORIGIN/..), so the addon loads wherever the package is unpacked."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
OUT = os.path.join(HERE, "lodestar_bls.node")
NODE_INCLUDE = os.environ.get("NODE_INCLUDE", "/usr/include/node")


def available() -> bool:
    return os.path.exists(os.path.join(NODE_INCLUDE, "node_api.h")) and shutil.which("g++") is not None


def build(force: bool = False, verbose: bool = False, out: str | None = None, lib_dir: str | None = None) -> str:
    """Build the addon.  By default into this directory against the package's library; with
    `out` / `lib_dir`, the same sources and flags into `out` against the liblodestar_bls.so in
    `lib_dir` (the tests link a stand-in library this way)."""
    src = os.path.join(HERE, "addon.cc")
    out = out or OUT
    rpath = os.path.abspath(lib_dir) if lib_dir else "$ORIGIN/.."
    lib_dir = lib_dir or PKG
    deps = [src, os.path.join(ROOT, "include", "lodestar_bls.h"), os.path.join(lib_dir, "liblodestar_bls.so")]
    if not force and os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(p) for p in deps):
        return out
    cmd = ["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
           "-DNODE_GYP_MODULE_NAME=lodestar_bls", f"-I{NODE_INCLUDE}", f"-I{os.path.join(ROOT, 'include')}",
           src, "-o", out + ".tmp", f"-L{lib_dir}", "-llodestar_bls", f"-Wl,-rpath,{rpath}", "-pthread"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(out + ".tmp", out)
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
