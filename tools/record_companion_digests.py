#!/usr/bin/env python
"""Record tests/golden/companion_digests.json: a sha256 of every output of every case of tests/companion_cases.py (needs the GPU).

The table pins the bits the companion kernels produce, so it is recorded from a build of the commit BEFORE a change to those kernels,
never from the code under test:

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/nerf_rpn_amd/csrc
    NRPN_LIBRARY=/tmp/parent/nerf_rpn_amd/libnerfrpn_hip.so python tools/record_companion_digests.py

tests/test_gpu_companion_bits.py then asserts that the in-tree library reproduces every digest.  `--out FILE` writes elsewhere.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from nerf_rpn_amd import lib  # noqa: E402
from companion_cases import run_all  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "companion_digests.json"))
    args = ap.parse_args()
    lib.call("check_device", 0)
    table = run_all(torch.device("cuda:0"))
    with open(args.out, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{args.out}: {len(table)} cases, {sum(len(v) for v in table.values())} digests, {os.path.getsize(args.out)} bytes "
          f"(recorded from {lib.SO_PATH})")


if __name__ == "__main__":
    main()
