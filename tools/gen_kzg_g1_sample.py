"""Write tests/golden/kzg_mainnet_g1_sample.json: 64 of the ceremony's G1 Lagrange points with
their indices in trusted_setup.txt (lines 0..31 and 4064..4095), for the test that fixes where
lb_kzg_load_setup_g1 applies the bit-reversal permutation.

    python tools/gen_kzg_g1_sample.py <trusted_setup.txt>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lodestar_amd import kzg  # noqa: E402


def main(path: str) -> None:
    with open(path) as f:
        g1 = kzg.parse_trusted_setup_g1(f.read())
    idx = list(range(32)) + list(range(4096 - 32, 4096))
    out = {"source": "trusted_setup.txt, G1 Lagrange lines (file order)",
           "points": [{"file_index": i, "g1": g1[48 * i:48 * i + 48].hex()} for i in idx]}
    dst = os.path.join(ROOT, "tests", "golden", "kzg_mainnet_g1_sample.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(dst, len(idx), "points")


if __name__ == "__main__":
    main(sys.argv[1])
