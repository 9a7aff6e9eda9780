"""adf::amFilter / adf::createAMFilter / adf::AdaptiveManifoldFilter of the header-only C++ adaptor: both branches compile
(the cv::Mat one against the declaration stubs), and on a GPU tests/cpp/test_am.cpp -- host Mats through the adaptor,
compared with the C-ABI call and with checksums recorded from the NumPy statement -- passes.  The recorded checksums are
checked against the statement here, without a GPU."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import am_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _compile():
    from addingdisparityfiltering_amd import _lib

    assert os.path.exists(_lib.LIB_PATH)
    exe = os.path.join(tempfile.mkdtemp(prefix="adf_am_"), "test_am")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-DADF_NO_OPENCV", "-I", os.path.join(ROOT, "include"),
                    os.path.join(CPP, "test_am.cpp"),
                    "-L", libdir, "-ladf_wls", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    return exe


def test_am_opencv_branch_typechecks():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-I", os.path.join(CPP, "opencv_stub"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(CPP, "typecheck_am_opencv.cpp")], check=True)


def test_am_program_compiles_without_opencv():
    assert os.path.exists(_compile())


def test_the_recorded_checksums_are_the_statements(adf):
    text = open(os.path.join(CPP, "test_am.cpp")).read()
    H, W = 45, 66
    y, x = np.mgrid[0:H, 0:W]
    src = (((x * 37 + y * 101) % 4001) - 2000 + np.where(x >= W // 2, 5000, 0)).astype(np.int16)
    p = adf.amPlan(16.0, 0.2, -1, W, H)
    for ch in (1, 3):
        joint = np.stack([np.minimum(255, (x // 6) * 40 + (y // 4) * 25 + (x * 7 + y * 13 + c * 29) % 9) for c in range(ch)], -1).astype(np.uint8)
        for adjust in (False, True):
            out = am_ref.am_filter(joint if ch == 3 else joint[..., 0], src, p, p["jtab"], adjust).astype(np.int64)
            assert "{%d, %d}" % (out.sum(), (out * (1 + (y * W + x) % 251)).sum()) in text


@pytest.mark.gpu
def test_am_program_passes_on_gpu():
    exe = _compile()
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout
