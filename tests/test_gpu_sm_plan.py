"""A same-message package's launch order, case by case: the raw stage-name sequence it leaves
once retired (lb_last_stage_times) against tests/golden/sm_stage_sequences.json, recorded by
tools/record_stage_sequences.py --sm before the package's buffers were carved from one layout
(bls_carve.h), the verdicts against the C oracle's, and an _agg call's signatures against the
Python restatement.  The cases are tests/sm_seq_helper.py's."""
import pytest

from tests import sm_agg_helper as A
from tests import sm_seq_helper as H
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
    names, valid, agg = H.run_case(name, loads)
    sigs, want = loads["retry" if H.CASES[name][-1] else "valid"]
    assert valid == want
    if agg is not None:
        jobs, verdicts, v = [], [], 0
        for n in H.JOB_SIZES:
            jobs.append((None, sigs[v:v + n], None))
            verdicts.append(want[v:v + n])
            v += n
        assert list(zip(*agg)) == A.expected_job_aggregates(jobs, verdicts, H.MASK, validate=False)
    assert names == GOLDEN[name]
