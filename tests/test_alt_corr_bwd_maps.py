"""Builds and runs the host check of the on-demand correlation lookup
backward's index maps (tests/host/alt_corr_bwd_maps_check.cpp): a CPU
re-enactment of the direct, tiled+spill and finalize pieces through
csrc/alt_corr_bwd_maps.h reproduces a plain loop's df1 / df2 exactly, and
every address formed -- for coordinates including +-1e6, +-inf and NaN --
is in bounds. A wrong map is a memory fault on the GPU, so this runs
without one. Also checks, compile-only, that the kernels use no scratch."""

import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(cxx, out, sanitize):
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-I", os.path.join(REPO, "csrc"),
           os.path.join(REPO, "tests", "host", "alt_corr_bwd_maps_check.cpp"),
           "-o", out]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined"]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_alt_corr_bwd_index_maps(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "alt_corr_bwd_maps_check")
    # a stand-alone program: the sanitizers link in directly. Fall back to
    # a plain build where the sanitizer runtimes are not installed.
    r = _compile(cxx, exe, True)
    if r.returncode != 0:
        r = _compile(cxx, exe, False)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "all address-map checks passed" in run.stdout


def test_alt_corr_bwd_kernels_have_no_scratch(tmp_path):
    """Register arrays indexed by a loop counter (df1 partials, f1 pieces,
    the tap list) stay in registers only while every index is a
    compile-time constant. Compiles the kernels for gfx950 and reads the
    compiler's own resource report."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    r = subprocess.run(
        [hipcc, "--offload-arch=gfx950", "-O3", "--cuda-device-only",
         "-I", os.path.join(REPO, "csrc"), "-c",
         os.path.join(REPO, "csrc", "alt_corr_bwd.hip"),
         "-o", str(tmp_path / "alt_corr_bwd.o"),
         "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S*alt_corr_bwd_\w+_kernel\S*)",
                       r.stderr)
    scratch = [int(v) for v in
               re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in
           re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    # direct x 8 channel counts x {atomics, no atomics}, scatter, finalize
    assert len(names) == 18 and len(scratch) == 18, r.stderr[-4000:]
    assert scratch == [0] * 18, list(zip(names, scratch))
    assert max(lds) <= 64 * 1024, list(zip(names, lds))
