"""Builds and runs the host check of the halo-staged weight-gradient
kernel's address maps (tests/host/wrw_halo_maps_check.cpp): every global
source in bounds or the zero page, every LDS address in bounds and aligned,
transposed reads bank-conflict-free, and a CPU emulation of
stage -> transposed read -> MFMA operand order reproducing dW and dbias of
a direct loop exactly. A wrong map is a memory fault on the GPU, so this
runs without one."""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compile(cxx, out, sanitize):
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-I", os.path.join(REPO, "csrc"),
           os.path.join(REPO, "tests", "host", "wrw_halo_maps_check.cpp"),
           "-o", out]
    if sanitize:
        cmd[4:4] = ["-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined"]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_wrw_halo_address_maps(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found")
    exe = str(tmp_path / "wrw_halo_maps_check")
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


def test_wrw_halo_kernel_has_no_scratch(tmp_path):
    """The kernel's inline-asm transposed reads are only safe while the
    compiler neither spills nor copies their destinations; a variant that
    starts using scratch is the first sign. Compiles the kernel for gfx950
    and reads the compiler's own resource report."""
    import re
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    r = subprocess.run(
        [hipcc, "--offload-arch=gfx950", "-O3", "--cuda-device-only",
         "-I", os.path.join(REPO, "csrc"), "-c",
         os.path.join(REPO, "csrc", "conv_wrw_halo.hip"),
         "-o", str(tmp_path / "conv_wrw_halo.o"),
         "-Rpass-analysis=kernel-resource-usage"],
        capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S*conv_wrw_halo_kernel\S*)",
                       r.stderr)
    scratch = [int(v) for v in
               re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == 3 and len(scratch) == 3, r.stderr[-4000:]
    assert scratch == [0, 0, 0], list(zip(names, scratch))
