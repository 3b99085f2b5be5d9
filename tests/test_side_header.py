"""The shared host side of the side calls (mvtopicmodel_amd/csrc/mvhdp_side.h), without a GPU: the parts of the header that need no
handle, compiled with the host compiler against a stub runtime (tests/native/hip_stub) into a program of its own
(tests/native/side_probe.cpp) under AddressSanitizer and UBSan, and run as a child process.  The program checks the argument checkers at
their edges and the order of their conditions, that StreamTimer destroys exactly the events it created on every way out, that the lane
order is a bijection, and that dispatch_T calls its function once for a legal T and never otherwise."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")


def test_side_probe(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "side_probe"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(NATIVE, "hip_stub"), "-I", os.path.join(ROOT, "mvtopicmodel_amd", "csrc"),
                           "-o", str(exe), os.path.join(NATIVE, "side_probe.cpp")])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout
