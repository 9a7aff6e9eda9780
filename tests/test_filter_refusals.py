"""The refusals of the five edge-aware filters -- weightedMedianFilter, guidedFilter, dtFilter, jointBilateralFilter,
rollingGuidanceFilter -- against the values recorded from the code before their host halves, their Python mirror and
their C++ adaptor were each restated once (tests/filter_refusal_cases.py has the matrix and the recorder,
tests/filter_refusals.json the values): the return code and adf_last_error() of every C entry, the code and text of
every AdfError of the Python mirror, all exact.  Every call is refused before a device is touched: no GPU is needed."""
import json

import pytest

import filter_refusal_cases as cases


@pytest.fixture(scope="module")
def recorded():
    with open(cases.FIXTURE) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def python_calls(adf):
    return cases.python_cases(adf)


def test_every_message_is_pinned(recorded):
    """Every fail( message of the five sources and of the check they share is reached by a case (or listed as
    unreachable without a device, with its reason)."""
    cases.check_coverage(recorded)


def test_python_cases_are_the_recorded_ones(recorded, python_calls):
    assert sorted(python_calls) == sorted(recorded["python"])


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_refusal(adf, recorded, name):
    from addingdisparityfiltering_amd import _lib
    case = cases.CASES[cases.CASE_NAMES.index(name)]
    assert cases.run_case(_lib.lib(), case) == recorded["c"][name]


@pytest.mark.parametrize("name", sorted(cases.TABLE_CASES))
def test_table_refusal(adf, recorded, name):
    from addingdisparityfiltering_amd import _lib
    assert cases.run_table_case(_lib.lib(), name) == recorded["c"][name]


def test_python_refusals(adf, recorded, python_calls):
    """One test for the mirror's 177 calls: each is microseconds, and a difference names its case."""
    got = {name: cases.run_python_case(adf, fn) for name, fn in python_calls.items()}
    wrong = {name: (got[name], recorded["python"][name]) for name in got if got[name] != recorded["python"][name]}
    assert not wrong, wrong
