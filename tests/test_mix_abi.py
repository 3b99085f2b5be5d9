"""The two entry points of the useVectorsLambda mix through every layer that needs no device: declared in include/mvhdp.h, listed in
ABI_SYMBOLS, exported by the library, wrapped by NativeSampler / NativeGroup, reachable from Java (no JDK here, so by inspection, as
tests/test_emb_jni.py does).  Argument and state errors need a handle: tests/test_gpu_vectors_mix.py."""
import os
import re

from mvtopicmodel_amd import _lib
from mvtopicmodel_amd.native import NativeGroup, NativeSampler
from tests.test_emb_jni import HDR, JAVA, SHIM, _entries

NAMES = ("mvhdp_set_vectors_mix", "mvhdp_get_vectors_mix")


def test_declared_listed_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*mvhdp_handle\b" % n, hdr), n
        assert n in _lib.ABI_SYMBOLS
    L = _lib.load_library()
    for n in NAMES:
        assert getattr(L, n) is not None
    assert [f for f, _ in _lib.PlanInputC._fields_][-3:] == ["vectors_mix", "kernel_registers_mix", "unassigned"]


def test_python_wrappers():
    for cls in (NativeSampler, NativeGroup):
        assert callable(getattr(cls, "set_vectors_mix"))
    assert callable(NativeSampler.get_vectors_mix)


def test_reachable_from_java():
    src = re.sub(r"//[^\n]*", "", open(SHIM).read())
    ent = _entries(src)
    java = open(JAVA).read()
    for native, fn, pub in (("nSetVectorsMix", NAMES[0], "setVectorsMix"), ("nGetVectorsMix", NAMES[1], "getVectorsMix")):
        params, body = ent[native]
        assert re.search(r"\b%s\s*\(" % fn, body), native
        for a in re.findall(r"jdoubleArray (\w+)", params):          # every array is checked against the handle's shape first
            assert re.search(r"bad_len\(env, %s\b" % a, body), (native, a)
        assert re.search(r"private static native \w+ %s\(" % native, java)
        assert re.search(r"public \w+ %s\(" % pub, java)


def test_documents_no_longer_say_the_mix_is_missing():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for f in ("include/mvhdp.h", "README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(root, f)).read()
        assert not re.search(r"mix\W+(of the sweep, which )?is not done yet", text), f
        assert not re.search(r"useVectorsLambda`? (stays|must be) 0", text), f
        assert "mvhdp_set_vectors_mix" in text or "set_vectors_mix" in text or "setVectorsMix" in text, f
