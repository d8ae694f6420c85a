"""Builds and runs the host check of the tap-folded conv path
(tests/host/conv_fold_plan_check.cpp): the envelope, the weight-gradient
plan and, by enumeration, the pack / dw / partials index maps of
csrc/conv_fold.h that the kernels run. A wrong map is an out-of-bounds
write on the GPU, so this runs without one."""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(cxx, out, sanitize):
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-I", os.path.join(REPO, "csrc"),
           os.path.join(REPO, "tests", "host", "conv_fold_plan_check.cpp"),
           "-o", out]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined"]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_conv_fold_maps_and_plan(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "conv_fold_plan_check")
    # a stand-alone program: the sanitizers link in directly. Fall back to
    # a plain build where the sanitizer runtimes are not installed.
    r = _compile(cxx, exe, True)
    if r.returncode != 0:
        r = _compile(cxx, exe, False)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "conv fold maps hold" in run.stdout
