"""The native side of the test scaffolding, in one place: the C sources under tests/native/ built into shared objects (once per process,
in a temporary directory), the ctypes pointer helpers of their wrappers, and the two fixtures that several test modules share.  A test
module takes a fixture by importing its name: from tests.native_build import fake_rccl  # noqa: F401.  Test infrastructure: no GPU, no
product code."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
RESTATEMENT = ("-O2", "-ffp-contract=off", "-shared", "-fPIC", "-std=gnu11")     # every *_ref.c: no contraction into fma, ever
_built = {}


def shared_object(sources, flags=RESTATEMENT, link=("-lm",)):
    """Path of the shared object gcc makes of tests/native/<sources> (one name or several) with `flags` in front of them and `link`
    behind; built at the first call, the same file for the same sources and flags afterwards."""
    sources = (sources,) if isinstance(sources, str) else tuple(sources)
    key = (sources, tuple(flags), tuple(link))
    if key not in _built:
        stem = os.path.splitext(sources[0])[0]
        so = os.path.join(tempfile.mkdtemp(prefix=stem + "_"), f"lib{stem}.so")
        subprocess.check_call(["gcc", *flags, *[os.path.join(NATIVE, s) for s in sources], "-o", so, *link])
        _built[key] = so
    return _built[key]


def ref_lib(name, *more_sources, extra_flags=(), link=("-lm",)):
    """tests/native/<name>.c (and the sources it calls into), loaded; the wrapper declares the argtypes"""
    return C.CDLL(shared_object((name + ".c",) + more_sources, RESTATEMENT + tuple(extra_flags), link))


def fake_rccl_lib():
    """tests/native/fake_rccl.c: the collectives of a shard group between processes of one machine, over shared memory"""
    return shared_object("fake_rccl.c", ("-O2", "-shared", "-fPIC", "-I/opt/rocm/include"),
                         ("-L/opt/rocm/lib", "-lamdhip64", "-lrt", "-lpthread", "-Wl,-rpath,/opt/rocm/lib"))


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def ptr_array(arrays):
    return (C.c_void_p * len(arrays))(*[None if a is None else a.ctypes.data for a in arrays])


@pytest.fixture(scope="module")
def fake_rccl():
    return fake_rccl_lib()


@pytest.fixture(scope="module")
def jvm(tmp_path_factory):
    """the test-side JNIEnv over the four shim sources as one translation unit"""
    from mvtopicmodel_amd import _lib
    from tests import jni_harness as H
    _lib.load_library()
    return H.Jvm(H.build_shim(tmp_path_factory.mktemp("one_tu_jni"), _lib.LIB_PATH, one_tu=True))
