#!/usr/bin/env python
"""Record tests/golden/conv_plans.npz: every conv size / plan query over the sweep of tests/conv_plan_sweep.py (host only, no GPU).

The table pins what the planning code decides, so it is recorded from a build of the commit BEFORE a change to that code, never from
the code under test:

    git worktree add /tmp/parent HEAD~1 && make -C /tmp/parent/nerf_rpn_amd/csrc
    NRPN_LIBRARY=/tmp/parent/nerf_rpn_amd/libnerfrpn_hip.so python tools/record_conv_plans.py

tests/test_conv_plans.py then asserts that the in-tree library reproduces every row.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from nerf_rpn_amd import lib  # noqa: E402
from conv_plan_sweep import sweep  # noqa: E402


def main():
    out = os.path.join(ROOT, "tests", "golden", "conv_plans.npz")
    table = sweep(lib.load())
    np.savez_compressed(out, **table)
    rows = sum(v.shape[0] for k, v in table.items() if k.endswith("_shapes"))
    print(f"{out}: {rows} shapes, {len(table) - 4} columns, {sum(v.size for v in table.values())} integers, {os.path.getsize(out)} bytes "
          f"(recorded from {lib.SO_PATH})")


if __name__ == "__main__":
    main()
