"""The refusals of the two matchers' C entries -- return code and adf_last_error(), exact -- against the values recorded
from the host code before it was restated as call record / check / plan / run (tests/matcher_refusal_cases.py has the
matrix and the recorder; tests/matcher_refusals.json the values).  A refused call leaves its output planes untouched; the
few accepted cases (a pair stride that only a device map must keep even) give the dense call's maps."""
import json

import pytest

import matcher_refusal_cases as cases


@pytest.fixture(scope="module")
def recorded():
    with open(cases.FIXTURE) as fh:
        return json.load(fh)


def test_every_message_is_pinned(recorded):
    """Every fail( message of the two host halves is reached by a case or listed as unreached with its reason."""
    cases.check_coverage(recorded)


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_refusal(adf, recorded, name):
    from addingdisparityfiltering_amd import _lib
    case = cases.CASES[cases.CASE_NAMES.index(name)]
    assert cases.run_case(_lib.lib(), case) == recorded[name]
