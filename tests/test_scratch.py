"""The call-scoped device array of the library's host side (mvtopicmodel_amd/csrc/mvhdp_scratch.h), without a GPU: the header compiled
with the host compiler against a stub runtime (tests/native/hip_stub) into a program of its own (tests/native/scratch_probe.cpp) under
AddressSanitizer and UBSan, and run as a child process.  The program checks the frees on every way out of a scope, the byte counts
handed to the runtime, the bounds of the copies and release(); a leak, a double free or a copy past an allocation ends it non-zero."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def test_scratch_probe(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "scratch_probe"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(NATIVE, "hip_stub"), "-I", os.path.join(ROOT, "mvtopicmodel_amd", "csrc"),
                           "-o", str(exe), os.path.join(NATIVE, "scratch_probe.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout
