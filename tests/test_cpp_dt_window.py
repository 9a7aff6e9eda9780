"""adf::dtWindowFilter / adf::createDTWindowFilter of the header-only C++ adaptor: both branches compile (the cv::Mat one
against the declaration stubs), and on a GPU tests/cpp/test_dt_window.cpp -- host Mats through the adaptor, compared with
the C-ABI call and with a small sequential restatement on two shapes -- passes."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _compile():
    from addingdisparityfiltering_amd import _lib

    assert os.path.exists(_lib.LIB_PATH)
    exe = os.path.join(tempfile.mkdtemp(prefix="adf_dtw_"), "test_dt_window")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-DADF_NO_OPENCV", "-I", os.path.join(ROOT, "include"),
                    os.path.join(CPP, "test_dt_window.cpp"),
                    "-L", libdir, "-ladf_wls", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    return exe


def test_dt_window_opencv_branch_typechecks():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-I", os.path.join(CPP, "opencv_stub"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(CPP, "typecheck_dt_window_opencv.cpp")], check=True)


def test_dt_window_program_compiles_without_opencv():
    assert os.path.exists(_compile())


@pytest.mark.gpu
def test_dt_window_program_passes_on_gpu():
    exe = _compile()
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout
