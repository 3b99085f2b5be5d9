"""The Java layer of the embeddings (no JDK here, so by inspection; tests/test_jni_shim.py type-checks the whole shim): every mvhdp_emb_*
entry point of include/mvhdp.h is reached from a JNI entry of mvtopicmodel_amd/java/mvhdp_jni.cpp, each of those has its native in
NativeSampler.java, and every array an entry takes is checked against the handle's shape before the library sees it.
(tests/test_jni_fake_jvm.py now RUNS every one of those length checks, one element short and one long, against a stand-in library, and
tests/test_gpu_jni.py runs the entries on a device: the regular expressions here stay as the check that needs no compiler.)"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "mvtopicmodel_amd", "java", "mvhdp_jni.cpp")
JAVA = os.path.join(ROOT, "mvtopicmodel_amd", "java", "org", "madgik", "MVTopicModel", "NativeSampler.java")
HDR = os.path.join(ROOT, "include", "mvhdp.h")


def _entries(src):
    """name -> body of every JNI entry of the shim"""
    out = {}
    for m in re.finditer(r"Java_org_madgik_MVTopicModel_NativeSampler_(n\w+)\(([^)]*)\)\s*\{", src):
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(src[i], 0)
            i += 1
        out[m.group(1)] = (m.group(2), src[m.end():i])
    return out


def test_every_embedding_entry_point_is_reachable_from_java():
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"\b(mvhdp_emb_[a-z_]+)\s*\(", hdr))
    assert len(declared) == 10
    src = re.sub(r"//[^\n]*", "", open(SHIM).read())
    ent = _entries(src)
    called = {n for _, body in ent.values() for n in re.findall(r"\b(mvhdp_emb_[a-z_]+)\s*\(", body)}
    assert declared == called
    natives = set(re.findall(r"private static native \w[\w\[\]]* (nEmb\w+)\(", open(JAVA).read()))
    assert natives == {n for n in ent if n.startswith("nEmb")} and len(natives) == 10
    assert re.search(r"public EmbStats embTrain\(", open(JAVA).read()) and "class EmbConfig" in open(JAVA).read()


def test_embedding_entries_check_every_array_length():
    src = re.sub(r"//[^\n]*", "", open(SHIM).read())
    for name, (params, body) in _entries(src).items():
        if not name.startswith("nEmb"):
            continue
        arrays = re.findall(r"j(?:int|long|double)Array (\w+)", params)
        for a in arrays:
            if name == "nEmbSamplingTable":                         # its length IS the range asked for; the library checks the range
                assert "GetArrayLength(types)" in body
                continue
            assert re.search(r"bad_len\(env, %s\b" % a, body), (name, a)
        if name not in ("nEmbInit", "nEmbCountWords", "nEmbTrain", "nEmbRelease"):
            assert "emb_missing(env, s)" in body, name             # the embedding shape is known before any length is checked
