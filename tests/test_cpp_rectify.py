"""initUndistortRectifyMap / remap / rectifyViews in the header-only C++ adaptor: both branches compile (the cv::Mat one
against the declaration stubs, with cv::Scalar and CV_32FC1 from tests/cpp/opencv_stub_rectify), the host-only part of
tests/cpp/test_rectify.cpp -- the parameter inverse and every refusal -- passes without a device, and on a GPU the whole
program -- the adaptor against a direct loop over the definition -- passes."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _compile():
    from addingdisparityfiltering_amd import _lib

    assert os.path.exists(_lib.LIB_PATH)
    exe = os.path.join(tempfile.mkdtemp(prefix="adf_rectify_"), "test_rectify")
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-DADF_NO_OPENCV", "-I", os.path.join(ROOT, "include"),
                    os.path.join(CPP, "test_rectify.cpp"), "-L", libdir, "-ladf_wls", "-Wl,-rpath," + libdir, "-o", exe], check=True)
    return exe


def _run(exe, *args):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, env=env, timeout=300)


def test_rectify_opencv_branch_typechecks():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-I", os.path.join(CPP, "opencv_stub_rectify"),
                    "-I", os.path.join(CPP, "opencv_stub_calib3d"), "-I", os.path.join(CPP, "opencv_stub_imgproc"),
                    "-I", os.path.join(CPP, "opencv_stub"), "-I", os.path.join(ROOT, "include"),
                    os.path.join(CPP, "typecheck_rectify_opencv.cpp")], check=True)


def test_rectify_program_host_part_passes_without_a_device():
    r = _run(_compile(), "--host-only")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host part passed" in r.stdout


@pytest.mark.gpu
def test_rectify_program_passes_on_gpu():
    r = _run(_compile())
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all passed" in r.stdout
