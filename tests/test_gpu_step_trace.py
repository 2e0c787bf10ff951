"""GPU: the launches of one training step -- every ``ops.call`` with its arguments and stream, every ``ops._conv_fwd`` /
``ops.conv_rows_fwd`` with its options -- must be the ones recorded in tests/golden/step_trace.json.gz (tests/step_trace.py), for the
eight configurations that between them reach every gradient-delivery path: sink / flat arena range / fused multi-weight GEMM / handed
back to autograd, side stream on and off, cone and dense RPN head, bf16 and bf16x3, Swin + FCOS norms and attention.

The golden file is re-recorded with ``python tests/step_trace.py --record``, and only by a change that MEANS to alter the launches of a
step; a refactor that moves a launch, an argument or a stream has changed behaviour and is fixed in the code."""
import pytest

import step_trace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return step_trace.load_golden()


@pytest.mark.parametrize("name", step_trace.CONFIGS)
def test_step_launches_match_the_recorded_trace(name, recorded, dev):
    import json
    r = step_trace.run(name, dev)
    got = json.loads(json.dumps(r["trace"]))
    print(f"[step_trace] {name}: {len(got)} launches, {r['seconds']:.1f} s, loss {r['loss']}, grad {r['grad']}")
    assert len(recorded[name]) > 200
    diff = step_trace.first_difference(got, recorded[name])
    assert diff is None, f"{name}: {diff}"
