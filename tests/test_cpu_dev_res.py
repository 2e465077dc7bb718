"""The owner of a handle's device memory, streams and events (csrc/dev_res.h) against a fake HIP runtime.

tests/host/dev_res_test.cpp is a stand-alone program: it defines the HIP entry points the header calls over malloc, runs
one scripted life of an owner clean and then once for every k with the k-th fake call failing, and checks after each run
that nothing is left alive or freed twice, that every failing step returned its documented code with an error text and left
its output untouched, and that the slots follow the one growth rule.  It then walks one host-pointer call of three segments
(the last one ragged) through the staging helper of the same header, again clean and with every fake call failing in turn:
inputs and outputs arrive at their rows, null arguments take no slot and no copy, an output kept on the device gets a slot
and is not copied out, device pointers are only offset, and the owner still releases everything.  It needs a host C++
compiler and the HIP headers, no GPU and no ROCm library."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owner_against_fake_runtime(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler on the path")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "dev_res_test")
    cmd = [cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           "-I" + os.path.join(ROOT, "industrial_nnmpc_2021_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host", "dev_res_test.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-2000:]
    assert "dev_res_test: ok" in ran.stdout
