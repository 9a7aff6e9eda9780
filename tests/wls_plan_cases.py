"""The case matrix of tests/test_gpu_wls_launch_plan.py and the recorder of its fixture.

A case is one DisparityWLSFilter call on tiny inputs by a fresh handle under the case's environment (the knobs are read
when a handle is created).  What is recorded is the launch plan as the library itself reports it: getLastSolver(),
getLastPath(), getLastSolverPath(), workspaceBytes() and, per kernel class of readProfile(), the launches and the
algorithmic and moved bytes (not the time).  All of it is a pure function of the host code in csrc/adf_api.hip.

    python tests/wls_plan_cases.py [output.json]

records tests/wls_launch_plan.json on a GPU.  The fixture pins the host code as it was BEFORE the call record / map
source / confidence stage refactor: it is never recorded again from later code, a difference is a bug in that code.

Views are 96 x 64 with an ROI whose x is odd (the confidence plane's cx0 != 0) and whose top and bottom offsets are
non-zero.  Two kinds of case leave that size or that ROI, for the reason they carry in `why`:
  * `big`: the merged preparation launch takes calls of up to 2.5e6 ROI pixels (conf_kernels.hip, prep_small_fits), so a
    full chunk of two pairs and a one-pair tail take different stages only when one pair's ROI has more than 1.25e6
    pixels -- at 96 x 64 both chunks are always merged.
  * `narrow`: the left-view confidence kernel writes the right-hand sides itself (int16 maps), or leaves them to the
    confidence-weighted prologue (float maps), only where the first row pass cannot be fused, which at aligned maps
    means an ROI of fewer than 4 columns.
A batch of 3 pairs runs under ADF_WS_LIMIT_GB = 2.2 x the per-pair workspace: a chunk of two pairs and a tail of one.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wls_launch_plan.json")

VIEW = (96, 64)                                   # W, H
# geometry -> (maps' size, ROI in map coordinates)
GEOMETRY = {
    "same": ((96, 64), (5, 3, 80, 56)),
    "half": ((48, 32), (3, 2, 40, 27)),          # view ROI (6, 4, 80, 54): even x >= 2, the half-width form applies
    "twice": ((192, 128), (11, 6, 160, 112)),    # view ROI (5, 3, 80, 56)
    "narrow": ((96, 64), (5, 3, 3, 56)),
    "big": ((1536, 1024), (5, 3, 1520, 1000)),   # view 1536 x 1024
}
KNOBS = ("ADF_MERGE_SMALL", "ADF_CONF_BAND", "ADF_SCALED_FUSE", "ADF_LO_HALF", "ADF_ROW_WEIGHTS_GUIDE", "ADF_NO_OVERLAP",
         "ADF_WS_LIMIT_GB")


def _case(name, geometry="same", conf=True, solver="wave", radius=2, maps="int16", out="int16", env=None, pairs=1,
          host=False, why=None):
    return dict(name=name, geometry=geometry, conf=conf, solver=solver, radius=radius, maps=maps, out=out,
                env=dict(env or {}), pairs=pairs, host=host, why=why)


CASES = [
    # ---- confidence on, same size ----
    _case("same-wave-r2"),
    _case("same-wave-r2-nomerge", env={"ADF_MERGE_SMALL": "0"}),
    _case("same-wave-r2-noband", env={"ADF_CONF_BAND": "0"}),
    _case("same-wave-r2-nomerge-nooverlap", env={"ADF_MERGE_SMALL": "0", "ADF_NO_OVERLAP": "1"}),
    _case("same-wave-r2-nomerge-chor", env={"ADF_MERGE_SMALL": "0", "ADF_ROW_WEIGHTS_GUIDE": "0"}),
    _case("same-wave-r9", radius=9),
    _case("same-wave-r9-chor", radius=9, env={"ADF_ROW_WEIGHTS_GUIDE": "0"}),
    _case("same-wave-r9-nooverlap", radius=9, env={"ADF_NO_OVERLAP": "1"}),
    _case("same-wave-r9-f32out", radius=9, out="float32"),
    _case("same-exact-r2-f32out", solver="exact", out="float32"),
    _case("same-exact-r9", solver="exact", radius=9),
    _case("same-exact-r2-nooverlap", solver="exact", env={"ADF_NO_OVERLAP": "1"}),
    _case("same-wave-r2-f32in-f32out", maps="float32", out="float32"),
    _case("same-wave-r2-f32in-nomerge", maps="float32", env={"ADF_MERGE_SMALL": "0"}),
    _case("same-wave-r2-f32in-noband", maps="float32", env={"ADF_CONF_BAND": "0"}),
    _case("same-wave-r9-f32in-f32out", radius=9, maps="float32", out="float32"),
    _case("same-exact-r2-f32in", solver="exact", maps="float32"),
    _case("same-exact-r9-f32in", solver="exact", radius=9, maps="float32"),
    _case("same-wave-r2-host", host=True),
    _case("same-wave-r2-f32in-host", maps="float32", host=True),
    _case("narrow-wave-r2", geometry="narrow", why="an unfused first row pass behind the left-view kernel needs < 4 ROI columns"),
    _case("narrow-wave-r2-f32in", geometry="narrow", maps="float32",
          why="the confidence-weighted prologue behind the left-view kernel needs < 4 ROI columns"),
    # ---- confidence on, maps at half the view's size ----
    _case("half-wave-r2", geometry="half"),
    _case("half-wave-r2-nohalf", geometry="half", env={"ADF_LO_HALF": "0"}),
    _case("half-wave-r2-nofuse", geometry="half", env={"ADF_SCALED_FUSE": "0"}),
    _case("half-wave-r2-noband", geometry="half", env={"ADF_CONF_BAND": "0"}),
    _case("half-wave-r2-noband-nofuse", geometry="half", env={"ADF_CONF_BAND": "0", "ADF_SCALED_FUSE": "0"}),
    _case("half-wave-r2-nooverlap", geometry="half", env={"ADF_NO_OVERLAP": "1"}),
    _case("half-wave-r9-f32out", geometry="half", radius=9, out="float32"),
    _case("half-wave-r2-f32in-f32out", geometry="half", maps="float32", out="float32"),
    _case("half-wave-r9-f32in", geometry="half", radius=9, maps="float32"),
    _case("half-exact-r2", geometry="half", solver="exact"),
    _case("half-exact-r2-f32in", geometry="half", solver="exact", maps="float32"),
    _case("half-wave-r2-host", geometry="half", host=True),
    # ---- confidence on, maps at twice the view's size ----
    _case("twice-wave-r2", geometry="twice"),
    _case("twice-wave-r9-f32in", geometry="twice", radius=9, maps="float32"),
    _case("twice-exact-r2-f32out", geometry="twice", solver="exact", out="float32"),
    # ---- confidence on, 3 pairs in a chunk of two and a tail of one ----
    _case("same-wave-r2-x3", pairs=3),
    _case("same-wave-r2-nomerge-x3", pairs=3, env={"ADF_MERGE_SMALL": "0"}),
    _case("same-wave-r9-x3", pairs=3, radius=9),
    _case("same-exact-r2-x3", pairs=3, solver="exact"),
    _case("same-wave-r2-f32in-x3", pairs=3, maps="float32"),
    _case("same-wave-r9-f32in-x3", pairs=3, radius=9, maps="float32"),
    _case("half-wave-r2-x3", geometry="half", pairs=3),
    _case("half-wave-r2-nofuse-x3", geometry="half", pairs=3, env={"ADF_SCALED_FUSE": "0"}),
    _case("half-wave-r2-f32in-x3", geometry="half", pairs=3, maps="float32"),
    _case("twice-wave-r2-x3", geometry="twice", pairs=3),
    _case("big-wave-r2-x3", geometry="big", pairs=3,
          why="a full chunk too large for the merged launch and a one-pair tail that takes it need > 1.25e6 ROI pixels per pair"),
    # ---- confidence off ----
    _case("noconf-same", conf=False),
    _case("noconf-same-f32in", conf=False, maps="float32"),
    _case("noconf-half", conf=False, geometry="half"),
    _case("noconf-half-f32in", conf=False, geometry="half", maps="float32"),
]
CASE_NAMES = [c["name"] for c in CASES]
assert len(set(CASE_NAMES)) == len(CASES)


def _inputs(case, seed=11):
    """(view, left maps, right maps or None, ROI): numpy arrays for a host case, CUDA tensors otherwise."""
    (dw, dh), roi = GEOMETRY[case["geometry"]]
    w, h = GEOMETRY["big"][0] if case["geometry"] == "big" else VIEW
    n = case["pairs"]
    rng = np.random.default_rng(seed)
    dt = np.float32 if case["maps"] == "float32" else np.int16
    view = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    dl = rng.integers(0, 40 * 16, (n, dh, dw)).astype(dt)
    dr = (-rng.integers(0, 40 * 16, (n, dh, dw))).astype(dt) if case["conf"] else None
    arrs = [view, dl, dr]
    if n == 1:
        arrs = [a[0] if a is not None else None for a in arrs]
    if not case["host"]:
        import torch
        arrs = [torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None for a in arrs]
    return arrs[0], arrs[1], arrs[2], roi


def _one_call(adf, case, setenv, inputs, extra_env=None):
    """One call of a fresh handle under the case's environment -> the handle."""
    for k in KNOBS:
        setenv(k, None)
    for k, v in dict(case["env"], **(extra_env or {})).items():
        setenv(k, v)
    f = adf.createDisparityWLSFilterGeneric(case["conf"])
    f.setSolver(adf.SOLVER_WAVE if case["solver"] == "wave" else adf.SOLVER_EXACT)
    f.setDepthDiscontinuityRadius(case["radius"])
    f.setSigmaColor(1.5)
    f.enableProfiling(True)
    view, dl, dr, roi = inputs
    call = f.filterFloat if case["out"] == "float32" else f.filter
    call(dl, view, None, dr, roi)
    f.sync()
    if not case["host"]:
        import torch
        torch.cuda.synchronize()
    return f


def run_case(adf, case, setenv):
    """Run `case` and return its record.  setenv(name, value or None) sets or removes an environment variable."""
    inputs = _inputs(case)
    extra = None
    if case["pairs"] > 1:
        # the limit applies to the per-chunk workspace alone: everything else a handle holds depends on the call's
        # pair count and not on the chunk, so two calls that differ in the chunk only differ by whole pairs of it
        whole = _one_call(adf, case, setenv, inputs).workspaceBytes()
        single = _one_call(adf, case, setenv, inputs, {"ADF_WS_LIMIT_GB": "1e-9"}).workspaceBytes()
        per_pair = (whole - single) / (case["pairs"] - 1)
        assert per_pair > 0, (case["name"], whole, single)
        extra = {"ADF_WS_LIMIT_GB": "%.12f" % (2.2 * per_pair / 2 ** 30)}
    f = _one_call(adf, case, setenv, inputs, extra)
    prof = f.readProfile()
    return dict(solver=f.getLastSolver(), path=f.getLastPath(), solver_path=f.getLastSolverPath(),
                workspace_bytes=f.workspaceBytes(),
                profile={k: dict(launches=int(v["launches"]), alg_bytes=float(v["alg_bytes"]), moved_bytes=float(v["moved_bytes"]))
                         for k, v in sorted(prof.items())})


def check_coverage(adf, recorded):
    """A condition on the matrix, from the recorded values themselves: every path and class is reached."""
    by = {c["name"]: c for c in CASES}
    assert sorted(recorded) == sorted(by), "the fixture and the case list differ"
    on = [n for n in recorded if by[n]["conf"]]
    for bit in ("PATH_CONF_BAND", "PATH_FUSED_FIRST_PASS", "PATH_MERGED_PREP", "PATH_SCALED_FUSED", "PATH_SCALED_HALF"):
        assert any(recorded[n]["path"] & getattr(adf, bit) for n in on), bit
    assert any(recorded[n]["solver_path"] & adf.PATH_ROW_WEIGHTS_GUIDE for n in on)
    assert any(not recorded[n]["solver_path"] & adf.PATH_ROW_WEIGHTS_GUIDE for n in on if by[n]["solver"] == "wave")
    for cls in ("fill_outside", "weights", "discontinuity", "lrc_confidence", "plain_prologue", "pass_h_first", "pass_h", "pass_v",
                "pass_v_last", "resize", "quantise_maps"):
        assert any(cls in recorded[n]["profile"] for n in on), cls
    assert {recorded[n]["solver"] for n in on} == {adf.SOLVER_WAVE, adf.SOLVER_EXACT}
    # every value of every axis with confidence on, and the four cases without
    for axis in ("solver", "radius", "maps", "out", "pairs"):
        assert {by[n][axis] for n in on} == {c[axis] for c in CASES}, axis
    assert {"same", "half", "twice"} <= {by[n]["geometry"] for n in on}
    assert {k for n in on for k in by[n]["env"]} == set(KNOBS) - {"ADF_WS_LIMIT_GB"}
    assert sorted((by[n]["geometry"], by[n]["maps"]) for n in recorded if not by[n]["conf"]) == \
        [("half", "float32"), ("half", "int16"), ("same", "float32"), ("same", "int16")]
    # 3 pairs: a chunk of two and a tail of one -- the last column pass runs once per chunk
    for n in recorded:
        assert recorded[n]["profile"]["pass_v_last"]["launches"] == (2 if by[n]["pairs"] == 3 else 1), n
    # the full chunk and the tail take different stages: the band kernel and a weight launch for the two pairs, the
    # merged launch (which computes the weights itself) for the last one
    big = recorded["big-wave-r2-x3"]
    assert big["path"] & adf.PATH_MERGED_PREP and big["path"] & adf.PATH_CONF_BAND
    assert big["profile"]["lrc_confidence"]["launches"] == 2 and big["profile"]["weights"]["launches"] == 1
    # ... while at 96 x 64 both are merged: no weight launch at all
    assert "weights" not in recorded["same-wave-r2-x3"]["profile"]


def _record(path):
    sys.path.insert(0, ROOT)
    import addingdisparityfiltering_amd as adf

    def setenv(k, v):
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v

    recorded = {}
    for case in CASES:
        recorded[case["name"]] = run_case(adf, case, setenv)
        print(case["name"], json.dumps(recorded[case["name"]]), flush=True)
    check_coverage(adf, recorded)
    with open(path, "w") as fh:
        json.dump(recorded, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    _record(sys.argv[1] if len(sys.argv) > 1 else FIXTURE)
