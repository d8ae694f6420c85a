"""Builds and runs the host check of the conv weight-gradient plan
(tests/host/conv_plan_check.cpp): for every shape class the plan's rules
name, (path, nchunk, partials-buffer elements, accumulate) as csrc/conv_gemm.h
computes them against a recorded table. The buffer size and the chunk count
bound what the partials kernels write, so this runs without a GPU."""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(cxx, out, sanitize):
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-I", os.path.join(REPO, "csrc"),
           os.path.join(REPO, "tests", "host", "conv_plan_check.cpp"),
           "-o", out]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined"]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_conv_wrw_plan_table(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "conv_plan_check")
    # a stand-alone program: the sanitizers link in directly. Fall back to
    # a plain build where the sanitizer runtimes are not installed.
    r = _compile(cxx, exe, True)
    if r.returncode != 0:
        r = _compile(cxx, exe, False)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "plan rows match" in run.stdout
