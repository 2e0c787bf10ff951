"""GPU: the companion kernels (BatchNorm, max-pool, upsample-add, subsample, residual joins, LayerNorm, GroupNorm, GELU, patch merge,
rotated RoIAlign) give the bits they gave before they moved onto the shared channels-last access layer (csrc/chanlast.cuh).

tests/golden/companion_digests.json holds a sha256 of every output of every case of tests/companion_cases.py, recorded
(tools/record_companion_digests.py) from a build of the commit before that change; the in-tree library must reproduce each one, with the
pool / BatchNorm fast paths on and off."""
import json
import os

import pytest

from companion_cases import cases, run_case

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "companion_digests.json")) as _f:
    WANT = json.load(_f)
CASES = dict(cases())


def test_every_case_is_recorded():
    assert sorted(WANT) == sorted(f"{name}/fast{fast}" for name in CASES for fast in (1, 0))
    assert all(len(v) >= 2 and all(len(d) == 64 for d in v.values()) for v in WANT.values())


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [1, 0], ids=["fast", "general"])
@pytest.mark.parametrize("name", list(CASES))
def test_companion_outputs_keep_their_bits(name, fast, dev):
    got = run_case(CASES[name], dev, fast)
    want = WANT[f"{name}/fast{fast}"]
    assert sorted(got) == sorted(want)
    bad = {k: (got[k][:16], want[k][:16]) for k in want if got[k] != want[k]}
    assert not bad, (name, fast, bad)
