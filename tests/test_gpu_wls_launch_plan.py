"""The launch plan of DisparityWLSFilter::filter, as the library itself reports it, against the values recorded from the
host code before its orchestration was restated (tests/wls_plan_cases.py has the matrix and the recorder;
tests/wls_launch_plan.json the values).  Solver, path bits, workspace bytes and launch counts are exact; the byte
counts of the profile are sums of doubles, so a regrouped sum may move the last bit: relative 1e-12."""
import json

import pytest

import wls_plan_cases as cases


@pytest.fixture(scope="module")
def recorded():
    with open(cases.FIXTURE) as fh:
        return json.load(fh)


def test_matrix_reaches_every_path(adf, recorded):
    cases.check_coverage(adf, recorded)


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_launch_plan(adf, recorded, monkeypatch, name):
    case = cases.CASES[cases.CASE_NAMES.index(name)]

    def setenv(k, v):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)

    got, exp = cases.run_case(adf, case, setenv), recorded[name]
    for key in ("solver", "path", "solver_path", "workspace_bytes"):
        assert got[key] == exp[key], (key, got[key], exp[key])
    assert sorted(got["profile"]) == sorted(exp["profile"])
    for cls, e in exp["profile"].items():
        g = got["profile"][cls]
        assert g["launches"] == e["launches"], (cls, g, e)
        for key in ("alg_bytes", "moved_bytes"):
            assert g[key] == pytest.approx(e[key], rel=1e-12, abs=0), (cls, key, g[key], e[key])
