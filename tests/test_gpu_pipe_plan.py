"""The pipeline's launch order, case by case: the raw stage-name sequence of one call
(lb_last_stage_times, one entry per launch) against tests/golden/pipeline_stage_sequences.json,
recorded by tools/record_stage_sequences.py before the call was split into plan, layout and
enqueue functions (bls_plan.h, run_pipeline), and the verdicts against the C oracle's.  The
cases -- every switch of the plan that moves a launch, on 130 sets in requests of 1, 2 and 127,
a lone 1,000-set call under the lone rule, a two-phase call -- are tests/pipe_seq_helper.py's."""
import pytest

from tests import pipe_seq_helper as H
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

GOLDEN = load_golden(H.FIXTURE)


@pytest.fixture(scope="module")
def loads(device):
    return H.workloads(device)


def test_fixture_covers_the_cases():
    assert sorted(GOLDEN) == sorted(H.CASES)


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_stage_sequence_and_verdicts(loads, name):
    names, valid, err = H.run_case(name, loads)
    _, _, want_valid, want_err = loads[H.CASES[name][1]]
    assert err == want_err and valid == want_valid
    assert names == GOLDEN[name]
