"""The JNI shim (the four sources of mvtopicmodel_amd/java, all 56 entries), compiled unmodified and RUN without a JVM and without a device.

tests/jni_harness.py links it with a test-side JNIEnv (tests/native/fake_jvm.cpp) and either the real libmvhdp.so -- which loads on a
machine without a device and answers MVHDP_ERR_NO_DEVICE -- or a stand-in (tests/native/fake_mvhdp.c) that logs and records what it
is handed.  Here: the fake's own self-tests, the prototype table against the shim's and the Java class's signatures, the refusals
that need no handle, and against the stand-in every length check of every entry, the lifecycle races, the tuning round trip and an
injected array failure -- for the entries of NativeSimilarity, NativePhrases and NativeHeldout as for NativeSampler's, and in both forms
a host may build the sources in (the four on one command line; one translation unit), since the handle registry is shared between them.
The same harness drives the real library on a device in tests/test_gpu_jni.py."""
import ctypes as C
import re
import subprocess
import threading
import time

import numpy as np
import pytest

from mvtopicmodel_amd import _lib
from tests import jni_harness as H
from tests.jni_harness import JavaException, JniGroup, JniSampler

IAE, ISE, RTE, OOM = ("java/lang/IllegalArgumentException", "java/lang/IllegalStateException", "java/lang/RuntimeException",
                      "java/lang/OutOfMemoryError")


class StandIn:
    def __init__(self, tmp):
        self.path = H.build_standin(tmp)
        self.fm = fm = C.CDLL(self.path)
        fm.fm_log_at.restype = C.c_char_p
        fm.fm_counter.argtypes = [C.c_char_p]
        fm.fm_group_member.restype = fm.fm_destroyed.restype = C.c_void_p
        self.jvm = H.Jvm(H.build_shim(tmp, self.path, name="libmvhdp_jni_standin.so"))                 # the four sources on one command line
        self.forms = {"four_sources": self.jvm, "one_tu": H.Jvm(H.build_shim(tmp, self.path, name="libmvhdp_jni_standin_one_tu.so", one_tu=True))}

    def reset(self, status=0):
        self.fm.fm_reset()
        self.fm.fm_set_status(status)
        self.fm.fm_block_sweeps(0)

    def log(self):
        return [self.fm.fm_log_at(i).decode() for i in range(self.fm.fm_log_len())]

    def counter(self, what):
        v = self.fm.fm_counter(what.encode())
        assert v != -12345, what
        return v


@pytest.fixture(scope="module")
def standin(tmp_path_factory):
    return StandIn(tmp_path_factory.mktemp("jni_standin"))


@pytest.fixture(scope="module")
def real(tmp_path_factory):
    _lib.load_library()                                       # (first: it picks the one HIP runtime of the process)
    return H.Jvm(H.build_shim(tmp_path_factory.mktemp("jni_real"), _lib.LIB_PATH))


@pytest.fixture
def jvm(standin):
    standin.reset()
    standin.jvm.lib.fj_ledger_reset()
    standin.jvm.lib.fj_exception_clear()
    return standin.jvm


def raises(cls, fn, *a, contains=None):
    with pytest.raises(JavaException) as e:
        fn(*a)
    assert e.value.cls == cls, str(e.value)
    if contains is not None:
        assert contains in e.value.msg, str(e.value)
    return e.value


# ---- the fake JVM, by hand ----
def test_fake_release_mode_0_copies_back_and_abort_does_not(jvm):
    a = jvm.ints([1, 2, 3])
    for mode, want in ((H.JNI_ABORT, [1, 2, 3]), (0, [7, 2, 3])):
        p = jvm.lib.fj_test_get_elements(a.h)
        assert p != jvm.lib.fj_array_data(a.h)                # always a copy
        C.cast(p, C.POINTER(C.c_int32))[0] = 7
        assert list(a.get()) == [1, 2, 3]                     # nothing reaches the array before the release
        assert jvm.ledger()["buffers_outstanding"] == 1
        jvm.lib.fj_test_release_elements(a.h, p, mode)
        assert list(a.get()) == want and jvm.ledger()["buffers_outstanding"] == 0
    assert not jvm.dirt()


def test_fake_ledger_sees_leaks_double_releases_and_damaged_guards(jvm):
    a, b = jvm.doubles([1.0, 2.0]), jvm.doubles([1.0, 2.0])
    p = jvm.lib.fj_test_get_elements(a.h)
    jvm.lib.fj_test_release_elements(b.h, p, 0)               # another array's buffer
    assert jvm.ledger()["bad_releases"] == 1 and jvm.ledger()["buffers_outstanding"] == 1
    jvm.lib.fj_test_release_elements(a.h, p, 0)
    jvm.lib.fj_test_release_elements(a.h, p, 0)               # released already
    assert jvm.ledger()["bad_releases"] == 2 and jvm.ledger()["buffers_outstanding"] == 0
    for at in (-1, 2):                                        # one element before, one past the end
        p = jvm.lib.fj_test_get_elements(a.h)
        C.cast(p, C.POINTER(C.c_double))[at] = 0.5
        jvm.lib.fj_test_release_elements(a.h, p, H.JNI_ABORT)
    assert jvm.ledger()["guard_damage"] == 2
    jvm.lib.fj_test_get_elements(a.h)                         # never released
    assert jvm.dirt() == {"buffers_outstanding": 1, "bad_releases": 2, "guard_damage": 2}
    jvm.lib.fj_ledger_reset()
    assert not jvm.dirt()


def test_fake_region_calls_are_bounded(jvm):
    a = jvm.ints([10, 11, 12, 13])
    buf = (C.c_int32 * 8)(*([-1] * 8))
    jvm.lib.fj_test_get_int_region(a.h, 1, 3, buf)
    assert list(buf)[:4] == [11, 12, 13, -1] and jvm.pending() is None
    jvm.lib.fj_test_get_int_region(a.h, 4, 0, buf)            # empty at the end: legal
    assert jvm.pending() is None
    for start, n in ((2, 3), (-1, 2), (0, 5), (5, 0), (1, -1)):
        buf = (C.c_int32 * 8)(*([-1] * 8))
        jvm.lib.fj_test_get_int_region(a.h, start, n, buf)
        assert jvm.take_exception()[0] == "java/lang/ArrayIndexOutOfBoundsException" and list(buf) == [-1] * 8
        jvm.lib.fj_test_set_int_region(a.h, start, n, buf)
        assert jvm.take_exception()[0] == "java/lang/ArrayIndexOutOfBoundsException" and list(a.get()) == [10, 11, 12, 13]
    assert jvm.ledger()["region_oob"] == 10
    d = jvm.doubles(3)
    jvm.lib.fj_test_get_int_region(d.h, 0, 1, buf)            # an int region of a double[]
    assert jvm.ledger()["misuse"] == 1


def test_fake_field_table_and_classes(jvm):
    o = jvm.object("t/Thing", "count:J,flag:I,ratio:D")
    assert jvm.lib.fj_test_set_long_field(o.h, b"count", b"J", 1 << 40) == 1 and o.get("count") == 1 << 40
    assert jvm.lib.fj_test_set_long_field(o.h, b"flag", b"I", -3) == 1 and o.get("flag") == -3
    assert jvm.lib.fj_test_set_long_field(o.h, b"ratio", b"D", 2) == 1 and o.get("ratio") == 2.0
    for name, sig in ((b"Count", b"J"), (b"count", b"I"), (b"flag", b"J")):     # a misspelt name, a wrong signature
        assert jvm.lib.fj_test_set_long_field(o.h, name, sig, 1) == 0
        cls, msg = jvm.take_exception()
        assert cls == "java/lang/NoSuchFieldError" and name.decode() in msg
    assert jvm.lib.fj_test_find_class(b"java/lang/IllegalStateException") == 1 and jvm.pending() is None
    assert jvm.lib.fj_test_find_class(b"org/madgik/MVTopicModel/NativeSampler") == 0      # the exception classes only
    assert jvm.take_exception()[0] == "java/lang/NoClassDefFoundError"
    assert not jvm.dirt()


def test_fake_counts_jni_calls_made_while_an_exception_is_pending(jvm):
    a, rows = jvm.ints(2), jvm.rows([[1.0], [2.0]])
    assert jvm.lib.fj_test_throw(b"java/lang/RuntimeException", b"first") == 0
    assert jvm.pending() == ("java/lang/RuntimeException", "first") and jvm.ledger()["calls_while_pending"] == 0
    p = jvm.lib.fj_test_get_elements(a.h)                     # forbidden
    assert jvm.ledger()["calls_while_pending"] == 1
    jvm.lib.fj_test_release_elements(a.h, p, 0)               # a release is allowed
    assert jvm.ledger()["calls_while_pending"] == 1
    assert jvm.lib.fj_test_array_length(a.h) == 2 and jvm.ledger()["calls_while_pending"] == 2
    jvm.lib.fj_exception_clear()
    r = jvm.lib.fj_test_object_element(rows.h, 1)
    jvm.lib.fj_test_throw(b"java/lang/RuntimeException", b"second")
    jvm.lib.fj_test_delete_local(r)                           # DeleteLocalRef is allowed
    assert jvm.ledger()["calls_while_pending"] == 2
    seen = []
    t = threading.Thread(target=lambda: seen.append(jvm.pending()))               # pending exceptions are per thread
    t.start(); t.join()
    assert seen == [None] and jvm.pending()[1] == "second"


def test_fake_local_references_and_injected_failures(jvm):
    rows = jvm.rows([[float(i)] for i in range(20)])
    jvm.lib.fj_begin_call()
    refs = [jvm.lib.fj_test_object_element(rows.h, i) for i in range(18)]
    for r in refs[:10]:
        jvm.lib.fj_test_delete_local(r)
    jvm.lib.fj_test_find_class(b"java/lang/RuntimeException")
    jvm.lib.fj_end_call()
    led = jvm.ledger()
    assert (led["locals_high_water"], led["locals_left"], led["local_arrays_left"]) == (18, 9, 8)
    assert set(jvm.dirt()) == {"local_arrays_left", "locals_high_water"}
    jvm.lib.fj_test_delete_local(refs[0])                     # deleted already
    assert jvm.ledger()["misuse"] == 1
    a = jvm.ints(3)
    jvm.fail_elements_at(2)
    p = jvm.lib.fj_test_get_elements(a.h)
    assert p and jvm.lib.fj_test_get_elements(a.h) is None and jvm.take_exception()[0] == OOM
    q = jvm.lib.fj_test_get_elements(a.h)                     # only the n-th
    assert q
    jvm.lib.fj_test_release_elements(a.h, p, 0); jvm.lib.fj_test_release_elements(a.h, q, 0)


# ---- the table, the Java class, the shim's source ----
def test_prototype_table_matches_the_shim_and_the_java_class():
    sig = H.shim_signatures()
    assert len(sig) == 56 and sig == H.PROTOTYPES
    assert H.java_natives() == H.PROTOTYPES
    per_class = {cls: sum(1 for v in sig.values() if v[2] == cls) for cls in H.CLASSES}
    assert per_class == {"NativeSampler": 51, "NativeSimilarity": 3, "NativePhrases": 1, "NativeHeldout": 1}


def test_the_fields_nSweep_asks_for_are_the_fields_of_SweepStats():
    src = open(H.SHIM).read()
    body = src[src.index(H.PREFIX["NativeSampler"] + "nSweep("):src.index(H.PREFIX["NativeSampler"] + "nApplyDelta(")]
    asked = {(name, {"L": "J", "I": "I", "D": "D"}[kind]) for kind, name in re.findall(r"set([LID])\(\"(\w+)\"", body)}
    java = open(H.JAVA["NativeSampler"]).read()
    cls = java[java.index("public static final class SweepStats"):]
    cls = cls[:cls.index("}")]
    declared = set()
    for typ, names in re.findall(r"public (long|int|double) ([^;]+);", cls):
        declared |= {(n.strip(), {"long": "J", "int": "I", "double": "D"}[typ]) for n in names.split(",")}
    assert len(asked) == 14 and asked == declared
    assert declared == {tuple(f.split(":")) for f in H.SWEEP_STATS_FIELDS.split(",")}


def test_the_stand_in_exports_what_the_shim_imports_and_the_fake_jvm_defines_the_rest(standin, tmp_path):
    imports, env = H.shim_imports(tmp_path)
    assert imports and env
    exported = {n for n in subprocess.check_output(["nm", "-D", "--defined-only", standin.path], text=True).split() if n.startswith("mvhdp_")}
    assert exported == imports
    assert imports <= set(_lib.ABI_SYMBOLS)
    defined = set(subprocess.check_output(["nm", "-D", "--defined-only", standin.jvm.path], text=True).split())
    assert env <= defined


# ---- against the real library: it loads here, and without a device it answers MVHDP_ERR_NO_DEVICE ----
def test_create_refuses_zero_and_nine_views(real):
    for V in ([], [5] * 9):
        raises(IAE, JniSampler, real, 10, V, contains="1..8 modalities")
    raises(IAE, real.call, "nCreate", 10, None, 0, 0)


def test_create_without_a_device_raises_the_librarys_message_and_registers_nothing(real):
    try:
        s = JniSampler(real, 10, [20, 30])
    except JavaException as e:
        assert e.cls == RTE and e.msg.startswith("mvhdp_create failed (-4): ") and "no usable HIP device" in e.msg, str(e)
        raises(ISE, real.call, "nBuildCounts", 0)
    else:                                                     # (a machine with a device: the handle is real)
        assert s.handle != 0
        s.close()
        raises(ISE, real.call, "nBuildCounts", s.handle or 1)


def _handle_argument_calls():
    """every entry that takes a handle or a group, with nothing but that argument filled in"""
    for name, (ret, codes, _) in H.PROTOTYPES.items():
        if name in ("nCreate", "nGroupUniqueId", "nGroupCreate"):
            continue
        assert codes[0] == "J"
        yield name, [0 if c in "JIDZ" else None for c in codes[1:]]


@pytest.mark.parametrize("bogus", [0, 0x5a5a5a5a5a58, -8])
def test_a_handle_that_was_never_issued_is_refused_not_dereferenced(real, bogus):
    real.log.clear()
    for name, rest in _handle_argument_calls():
        if name in ("nDestroy", "nGroupDestroy"):
            real.call(name, bogus)                            # close() of what is not open: nothing happens
        else:
            e = raises(ISE, real.call, name, bogus, *rest)
            assert e.msg in ("NativeSampler is closed", "group is closed"), (name, e.msg)
    raises(ISE, real.call, "nGroupCreate", real.longs([bogus]), contains="a member is closed")
    assert set(real.log) == set(H.PROTOTYPES) - {"nCreate", "nGroupUniqueId"}


# ---- against the stand-in ----
K, V, D, NTOK, EC, TOPN, HL = 5, [7, 4], 3, [6, 4], 3, 2, 3
M = len(V)
R = V[0] + K
DOC_OFF = [[0, 2, 2, 6], [0, 1, 3, 4]]
SN, SD, CAP, CW = 4, 3, 6, 7                                  # similarPairs: rows, columns; the capacity of the pair / phrase arrays; of the phrases' words


class A:
    """an array argument of a well-formed call: kind, the length the shim asks for, the words its refusal must carry (None: any length
    goes), whether null is allowed; rows: the length of each row of a double[][]"""

    def __init__(self, kind, n, label, nullable=False, rows=None, values=None):
        self.kind, self.n, self.label, self.nullable, self.rows, self.values = kind, n, label, nullable, rows, values

    def make(self, jvm, n=None):
        n = self.n if n is None else n
        if self.kind == "L":
            return jvm.rows([np.ones(self.rows)] * n)
        if self.values is not None and n == self.n:
            return jvm.array(self.kind, self.values)
        return jvm.array(self.kind, np.ones(n))


def _diag(prefix):
    return [TOPN, A("I", V[0], "diagnostics wordLength", True), A("D", 13 * K, "diagnostics scores"), A("D", 13 * K * TOPN, "diagnostics wordScores"),
            A("I", K * TOPN * TOPN, "diagnostics codoc"), A("I", K * TOPN, "diagnostics topTypes"), A("I", K * TOPN, "diagnostics topCounts"),
            A("I", K, "diagnostics nonzero"), A("I", K, "diagnostics rank1Docs"), A("I", K, "diagnostics nonzeroDocs"),
            A("I", K * 7, "diagnostics atProportions"), A("D", K, "diagnostics sumCountLogCount"), A("I", V[0], "diagnostics wordTypeCounts"),
            A("J", 1, "diagnostics numTokens"), A("D", M, "diagnostics perView")]


# a well-formed call of every entry that takes arrays, on the model below ("h": the handle, "g": the group)
GOOD = {
    "nSetCorpus": ["h", 0, A("J", D + 1, None, values=DOC_OFF[0]), A("I", NTOK[0], "setCorpus tokens")],
    "nSetAssignments": ["h", 0, A("I", NTOK[0], "setAssignments")],
    "nGetAssignments": ["h", 1, A("I", NTOK[1], "getAssignments")],
    "nSetViewPresence": ["h", 1, A("Z", D, "setViewPresence", True)],
    "nSetHyper": ["h", A("L", M, "setHyper alpha", rows=K + 1), A("D", M, "setHyper alphaSum"), A("D", M, "setHyper beta"), A("D", M, "setHyper betaSum"),
                  A("D", M, "setHyper gamma"), A("L", M, "setHyper p_a", rows=M), A("L", M, "setHyper p_b", rows=M), A("Z", K, "setHyper inactive", True)],
    "nGetCounts": ["h", 1, A("I", V[1] * K, "getCounts typeTopicCounts", True), A("I", K, "getCounts tokensPerTopic", True)],
    "nGetDocTopicHist": ["h", 0, A("I", K * HL, "getDocTopicHist hist", True), HL, A("I", 9, None, True)],
    "nGetAlpha": ["h", A("D", M * (K + 1), "getAlpha alpha"), A("Z", K, "getAlpha inactive")],
    "nSweep": ["h", 3, 77, 4, A("D", D * M * M, "sweep pOverride [D][M][M]", True), "stats"],
    "nModelLogLikelihood": ["h", A("D", M, "modelLogLikelihood")],
    "nSweepMany": ["h", 2, 3, 78, 4, A("J", 3 * 8, "sweepMany stats [n][8]", True)],
    "nGetTuning": ["h", A("I", 8, "getTuning ints"), A("D", 17, "getTuning doubles")],
    "nSetTuning": ["h", A("I", 8, "setTuning ints", values=[4, 1, 1, 1, 1, 3, 7, 11]), A("D", 17, "setTuning doubles", values=[0.5] * 17)],
    "nGroupUniqueId": [A("B", 128, "groupUniqueId")],
    "nGroupSweep": ["g", 1, 79, 0x20, A("J", 8, "groupSweep stats [members][8]", True), A("I", 3, "groupSweep act", True)],
    "nGetCountHistogram": ["h", 0, A("I", 11, None)],
    "nViewOverlapSums": ["h", A("D", M * M, "viewOverlapSums")],
    "nGammaDocStatistics": ["h", 1, 1.5, 80, 2, A("D", 2, "gammaDocStatistics")],
    "nDpTableStatistics": ["h", 1, A("I", K * HL, "dpTableStatistics hist [K][histLen]"), HL, A("D", K, "dpTableStatistics conc"), 81, 3,
                           A("D", K, "dpTableStatistics mk"), A("B", K, "dpTableStatistics active")],
    "nGroupModelLogLikelihood": ["g", A("D", M, "groupModelLogLikelihood")],
    "nGroupGetDocTopicHist": ["g", 1, A("I", K * HL, "groupGetDocTopicHist hist [K][histLen]", True), HL, A("I", 9, None, True)],
    "nGroupGetCountHistogram": ["g", 1, A("I", 11, None)],
    "nGroupViewOverlapSums": ["g", A("D", M * M, "groupViewOverlapSums [M][M]")],
    "nGroupGammaDocStatistics": ["g", 1, 1.5, 82, 2, A("D", 2, "groupGammaDocStatistics")],
    "nTopWords": ["h", 1, TOPN, A("I", K * TOPN, "topWords types"), A("I", K * TOPN, "topWords counts"), A("I", K, "topWords nonzero")],
    "nDiscrWeights": ["h", A("D", M, "discrWeights perView"), 1, A("D", V[1], "discrWeights typeWeight", True)],
    "nDiagnostics": ["h"] + _diag("diagnostics"),
    "nGroupDiagnostics": ["g"] + _diag("diagnostics"),
    "nEmbInit": ["h", A("I", 7, "embInit ints", values=[EC, 1, 1, 5, 5, 10, 1000]), 1000, A("D", 3, "embInit doubles", values=[1e-4, -6.0, 6.0]),
                 A("D", R * EC, "embInit weights [R*C]", True), 9],
    "nEmbTrain": ["h", 1, 83, 0, 1, A("J", 7, "embTrain longs"), A("D", 3, "embTrain doubles")],
    "nEmbGetVectors": ["h", A("D", R * EC, "embGetVectors weights", True), A("D", R * EC, "embGetVectors negativeWeights", True)],
    "nEmbSetVectors": ["h", A("D", R * EC, "embSetVectors weights", True), A("D", R * EC, "embSetVectors negativeWeights", True)],
    "nEmbWordStats": ["h", A("J", V[0], "embWordStats counts", True), A("D", V[0], "embWordStats retention", True), A("J", 1, "embWordStats totalWords")],
    "nEmbSamplingTable": ["h", 5, A("I", 6, None)],
    "nEmbSoftmax": ["h", 1, A("D", K * V[0], "embSoftmax expDot [K*V_0]", True), A("D", K, "embSoftmax sumExp", True)],
    "nEmbNearest": ["h", A("D", EC, "embNearest query"), TOPN, A("I", TOPN, "embNearest words"), A("D", TOPN, "embNearest wordSims"),
                    A("I", TOPN, "embNearest topics", True), A("D", TOPN, "embNearest topicSims", True)],
    "nSetVectorsMix": ["h", 0.5, A("D", K * V[0], "setVectorsMix expDot [K*V_0]", "pair"), A("D", K, "setVectorsMix sumExp", "pair")],
    "nGetVectorsMix": ["h", A("D", V[0] * K, "getVectorsMix mix [V_0*K]", True)],
    # NativeSimilarity, NativePhrases, NativeHeldout (the capacity arrays -- i, topics, counts, words -- go with any length)
    "nSimilarPairs": ["h", 1, SN, SD, A("D", SN * SD, "similarPairs xFlat"), 0.03, 0.15, 0, 0, A("I", CAP, None), A("I", CAP, "similarPairs j"),
                      A("D", CAP, "similarPairs sim"), A("J", 5, "similarPairs statsOut", True), A("D", 1, "similarPairs marginOut", True)],
    "nDocTopicsTop": ["h", A("D", M, "docTopicsTop viewWeights"), 0, D, 0.03, 3, A("J", D + 1, "docTopicsTop rowOff", True), A("I", CAP, None),
                      A("D", CAP, "docTopicsTop weights")],
    "nEntityTopicDistributions": ["h", A("D", M, "entityTopicDistributions viewWeights"), 0.03, -1, 5, A("J", 3, None, values=[0, 2, 3]),
                                  A("J", 3, None, values=[0, 1, 2]), A("D", 2 * K, "entityTopicDistributions out")],
    "nTopicPhrases": ["h", 20, 0, A("J", K + 1, "topicPhrases topicOff", True), A("J", CAP + 1, "topicPhrases wordOff"), A("I", CW, None, True), A("I", CAP, None),
                      A("J", K, "topicPhrases distinct", True), A("J", K, "topicPhrases occurrences", True), A("J", 2, "topicPhrases sizesOut"),
                      A("J", 5, "topicPhrases statsOut", True)],
    "nLeftToRight": ["h", 0, 3, 1, 17, 0, A("D", K, "heldout alpha", True), 0.0, A("J", D + 1, None, values=[0, 2, 2, 5]), A("I", 5, "heldout tokens"),
                     A("D", D, "heldout docLl", True), A("D", 5, "heldout positionSum", True), A("J", D, "heldout docTokens", True),
                     A("J", 3, "heldout statsOut", True)],
}
assert set(H.SIDE_ENTRIES) <= set(GOOD)
NO_ARRAYS = {"h": ["nBuildCounts", "nBuildTrees", "nEmbCountWords"], "g": ["nGroupBuildCounts", "nGroupDrain", "nGroupAbort"]}


class Model:
    """a sampler with its corpus and an embedding, and a group of it, on the stand-in (which answers MVHDP_OK and does nothing)"""

    def __init__(self, standin):
        self.standin, self.jvm = standin, standin.jvm
        standin.reset(0)
        self.s = JniSampler(self.jvm, K, V, device=2, docIdBase=1 << 33)
        for m in range(M):
            self.s.setCorpus(m, DOC_OFF[m], np.arange(NTOK[m]) % V[m])
        self.s.embInit(H.EmbConfig(numColumns=EC, numContextColumns=1, samplingTableSize=1000), None, 9)
        self.group = JniGroup(self.jvm, [self.s])
        self.stats = self.jvm.object(H.SWEEP_STATS_CLASS, H.SWEEP_STATS_FIELDS)

    def args(self, name, change=None):
        """the arguments of GOOD[name]; change = (index, length or None): that array with another length, or null"""
        out = []
        for i, a in enumerate(GOOD[name]):
            if isinstance(a, A):
                if change and change[0] == i:
                    out.append(None if change[1] is None else a.make(self.jvm, change[1]))
                else:
                    out.append(a.make(self.jvm))
            else:
                out.append({"h": self.s.handle, "g": self.group.g, "stats": self.stats}.get(a, a) if isinstance(a, str) else a)
        return out

    def close(self):
        self.group.close()
        self.s.close()


@pytest.fixture
def model(standin, jvm, tmp_path):
    m = Model(standin)
    m.tmp = tmp_path
    yield m
    standin.fm.fm_block_sweeps(0)
    standin.fm.fm_set_status(0)
    m.close()


def test_create_and_set_corpus_hand_the_library_what_java_handed_them(standin, model):
    cfg = _lib.Config()
    standin.fm.fm_create_config(C.byref(cfg))
    assert (cfg.num_topics, cfg.num_modalities, list(cfg.num_types), cfg.device, cfg.doc_id_base, cfg.flags) == (K, M, V + [0] * 6, 2, 1 << 33, 0)
    got = (C.c_int64 * 3)()
    standin.fm.fm_corpus(got)
    assert (standin.counter("corpus_m"), list(got)) == (M - 1, [D, NTOK[1], 0])
    model.s.setCorpus(0, [0, 0, 0], [])                       # no tokens at all: the library sees a null pointer, as the header allows
    assert standin.counter("corpus_tokens_null") == 1
    raises(IAE, model.s.call, "nSetCorpus", 0, None, None, contains="bad view or docOff")
    raises(IAE, model.s.call, "nSetCorpus", 0, model.jvm.longs([]), None, contains="bad view or docOff")
    raises(IAE, model.s.call, "nSetCorpus", M, model.jvm.longs([0, 1]), model.jvm.ints([0]), contains="bad view")


def test_every_length_check_of_every_entry(standin, model):
    checked = 0
    for name, spec in GOOD.items():
        for i, a in enumerate(spec):
            if not isinstance(a, A) or a.label is None:
                continue
            variants = [a.n + 1] + ([a.n - 1] if a.n > 0 else []) + ([None] if a.nullable is not True else [])
            for n in variants:
                if n is None and a.nullable == "pair":
                    continue
                before = standin.fm.fm_log_len()
                e = raises(IAE, model.jvm.call, name, *model.args(name, (i, n)))
                assert a.label in e.msg, (name, i, n, e.msg)
                assert f"length {a.n} expected, got {-1 if n is None else n}" in e.msg, (name, e.msg)
                assert standin.fm.fm_log_len() == before, f"{name}: {standin.log()[before:]} called although argument {i} was refused"
                checked += 1
            if a.nullable is True:                            # null is a value the header allows: the call goes through
                before = standin.fm.fm_log_len()
                model.jvm.call(name, *model.args(name, (i, None)))
                assert standin.fm.fm_log_len() > before, (name, i)
    assert checked >= 190, checked
    # the rows of the double[][] arguments of setHyper: alpha[m] holds K + 1 entries, p_a[m] / p_b[m] hold M
    for i, want, label in ((1, K + 1, "setHyper alpha[m]"), (6, M, "setHyper p_a[m]"), (7, M, "setHyper p_b[m]")):
        for n in (want - 1, want + 1, None):
            for row in range(M):
                args = model.args("nSetHyper")
                rows = [np.ones(want) for _ in range(M)]
                rows[row] = None if n is None else np.ones(n)
                args[i] = model.jvm.rows(rows)
                before = standin.fm.fm_log_len()
                e = raises(IAE, model.jvm.call, "nSetHyper", *args)       # (call() has checked: no row reference is left behind)
                assert label in e.msg and standin.fm.fm_log_len() == before
                assert model.jvm.last_ledger["locals_left"] == 1          # the exception's class
    # setVectorsMix: the two arrays go together
    for i in (2, 3):
        before = standin.fm.fm_log_len()
        raises(IAE, model.jvm.call, "nSetVectorsMix", *model.args("nSetVectorsMix", (i, None)), contains="go together")
        assert standin.fm.fm_log_len() == before
    args = model.args("nSetVectorsMix"); args[2] = args[3] = None
    model.jvm.call("nSetVectorsMix", *args)
    assert standin.log()[-1] == "mvhdp_set_vectors_mix"
    # arrays whose length is the caller's: null and the empty array
    for name in ("nGetCountHistogram", "nGroupGetCountHistogram"):
        for n in (None, 0):
            before = standin.fm.fm_log_len()
            raises(IAE, model.jvm.call, name, *model.args(name, (2, n)))
            assert standin.fm.fm_log_len() == before
    raises(IAE, model.jvm.call, "nEmbSamplingTable", *model.args("nEmbSamplingTable", (2, None)), contains="types is null")
    raises(IAE, model.jvm.call, "nGroupCreate", None, contains="no members")
    raises(IAE, model.jvm.call, "nGroupCreate", model.jvm.longs([]), contains="no members")
    # groupCreateRank's id (128 bytes): it is refused with the member already pinned, so the refusal has to give the pin back --
    # close() of the member returns (it would wait for ever on a pin nobody holds)
    for n in (127, 129, None):
        member = JniSampler(model.jvm, K, V)
        before = standin.fm.fm_log_len()
        e = raises(IAE, model.jvm.call, "nGroupCreateRank", member.handle, None if n is None else model.jvm.array("B", np.ones(n)), 0, 1)
        assert "groupCreateRank id" in e.msg and f"length 128 expected, got {-1 if n is None else n}" in e.msg, e.msg
        assert standin.fm.fm_log_len() == before, f"{standin.log()[before:]} called although the id was refused"
        destroy_returns(standin, model.jvm, member)


def test_scalar_arguments_out_of_range_are_refused_before_the_library(standin, model):
    bad = [("nSetAssignments", 1, M), ("nSetAssignments", 1, -1), ("nGetAssignments", 1, M), ("nSetViewPresence", 1, M), ("nGetCounts", 1, M),
           ("nGetDocTopicHist", 1, -1), ("nGetDocTopicHist", 3, 0), ("nGetCountHistogram", 1, M), ("nDpTableStatistics", 1, M), ("nDpTableStatistics", 3, 0),
           ("nGroupGetDocTopicHist", 1, M), ("nGroupGetDocTopicHist", 3, 0), ("nGroupGetCountHistogram", 1, -1), ("nGroupGammaDocStatistics", 1, M),
           ("nTopWords", 2, 0), ("nTopWords", 2, 65), ("nDiscrWeights", 2, M), ("nDiagnostics", 1, 0), ("nDiagnostics", 1, 65), ("nGroupDiagnostics", 1, 65),
           ("nEmbNearest", 2, 0), ("nEmbNearest", 2, 65), ("nSimilarPairs", 2, -1), ("nSimilarPairs", 3, 0), ("nDocTopicsTop", 2, -1), ("nDocTopicsTop", 3, D + 1)]
    for name, i, v in bad:
        args = model.args(name)
        args[i] = v
        before = standin.fm.fm_log_len()
        raises(IAE, model.jvm.call, name, *args)
        assert standin.fm.fm_log_len() == before, name
    args = model.args("nSweepMany"); args[2] = -1
    before = standin.fm.fm_log_len()
    model.jvm.call("nSweepMany", *args)                       # (n < 0: nothing to do, nothing called)
    assert standin.fm.fm_log_len() == before


def test_sweep_fills_all_fourteen_fields_and_sweep_many_the_flat_layout(standin, model):
    p = np.arange(D * M * M) + 0.25
    st = model.s.sweep(3, (1 << 40) + 5, 0x24, p)
    b = 1000 * 4
    assert [st.tokens, st.changed, st.newMassCnt, st.topicDocMassCnt, st.wordFTreeMassCnt, st.oovSkipped, st.abortedDocs, st.exactFallbacks,
            st.activatedTopic, st.activatedModality, st.activationKey, st.sweepKernelMs, st.totalMs, st.activations] == \
        [b + 1, b + 2, b + 3, b + 4, b + 5, b + 6, b + 7, b + 8, b + 9, b + 10, b + 11, b + 12.5, b + 13.5, b + 14]
    got, gp = (C.c_int64 * 3)(), (C.c_double * 2)()
    standin.fm.fm_sweep_args(got, gp)
    assert list(got) == [3, (1 << 40) + 5, 0x24] and gp[0] == 0.25 and standin.counter("sweep_has_p") == 1
    model.s.sweep(0, 1, 0, None)
    assert standin.counter("sweep_has_p") == 0
    sts = model.s.sweepMany(2, 3, 9, 0x4)
    for i, st in enumerate(sts):
        b = 1000 * (2 + i + 1)
        assert [st.tokens, st.changed, st.newMassCnt, st.topicDocMassCnt, st.wordFTreeMassCnt, st.oovSkipped, st.abortedDocs, st.exactFallbacks] == \
            [b + 1, b + 2, b + 3, b + 4, b + 5, b + 6, b + 7, b + 8]
    standin.fm.fm_sweep_args(got, gp)
    assert list(got) == [2, 9, 4] and standin.counter("sweep_n") == 3
    assert model.s.sweepMany(0, 0, 9, 0) == []


def test_outputs_come_back_and_scalars_keep_their_order(standin, model):
    nwk, nk = model.s.getCounts(1, V[1], K)
    assert (nwk[0, 0], nk[0]) == (41, 43)                     # what the library wrote into the buffers reaches the Java arrays
    model.s.topWords(1, TOPN, K)
    assert (standin.counter("top_m"), standin.counter("top_n")) == (1, TOPN)
    # the scalars the entries of the three other classes read back from the library
    args = model.args("nSimilarPairs")
    assert model.jvm.call("nSimilarPairs", *args) == 3
    assert list(args[-2].get()) == [101, 102, 103, 104, 105] and args[-1].get()[0] == 0.625
    assert model.jvm.call("nDocTopicsTop", *model.args("nDocTopicsTop")) == 2
    args = model.args("nTopicPhrases")
    assert model.jvm.call("nTopicPhrases", *args) == 3
    assert list(args[-2].get()) == [3, 5] and list(args[-1].get()) == [201, 202, 203, 204, 205]
    args = model.args("nLeftToRight")
    assert model.jvm.call("nLeftToRight", *args) == -12.5 and list(args[-1].get()) == [301, 302, 303]


def test_a_library_error_becomes_a_runtime_exception_with_its_message(standin, model):
    standin.fm.fm_set_status(-2)
    e = raises(RTE, model.s.buildCounts)
    assert e.msg == "mvhdp_build_counts failed (-2): the stand-in's message"
    e = raises(RTE, model.group.buildCounts)
    assert e.msg == "mvhdp_group_build_counts failed (-2): the stand-in's group message"
    for name in GOOD:                                         # every entry with arrays: the error path releases what it took (call() checks)
        if name == "nEmbInit":                                    # (its failure forgets the embedding: a test of its own below)
            continue
        raises(RTE, model.jvm.call, name, *model.args(name))


def destroy_returns(standin, jvm, sampler):
    """nDestroy of a handle nothing should hold any more: on its own thread, so that a pin left behind fails the test instead of hanging it"""
    destroyed = standin.counter("destroys")
    t, box = _in_thread(jvm.call, "nDestroy", sampler.handle)
    t.join(30)
    assert not t.is_alive(), "nDestroy waits for a pin that was never given back"
    assert "error" not in box and standin.counter("destroys") == destroyed + 1


def test_a_create_the_library_refuses_leaves_nothing_registered_and_nothing_pinned(standin, jvm):
    """mvhdp_create, mvhdp_group_create and mvhdp_group_create_rank failing: the library's message comes back, no handle or group is
    handed out, and the members a group entry had pinned are free again (their close() returns)."""
    standin.reset(-2)
    e = raises(RTE, JniSampler, jvm, K, V)
    assert e.msg == "mvhdp_create failed (-2): the stand-in's message" and standin.counter("creates") == 1
    standin.reset(0)
    a, b, c = (JniSampler(jvm, K, V) for _ in range(3))
    standin.fm.fm_set_status(-2)
    e = raises(RTE, JniGroup, jvm, [a, b])
    assert e.msg == "mvhdp_group_create failed (-2): the stand-in's group message"
    assert standin.counter("group_creates") == 1 and standin.counter("group_n") == 2
    e = raises(RTE, JniGroup.ofRank, jvm, c, np.zeros(128), 0, 1)
    assert e.msg == "mvhdp_group_create_rank failed (-2): the stand-in's group message" and standin.log()[-2] == "mvhdp_group_create_rank"
    standin.fm.fm_set_status(0)
    assert standin.counter("group_destroys") == 0             # (nothing was made, nothing is destroyed)
    for s in (a, b, c):
        s.buildCounts()                                       # the members are still open ...
        destroy_returns(standin, jvm, s)                      # ... and nobody holds them


def test_sweep_with_view_weights_before_any_corpus_is_a_state_error(standin, jvm):
    standin.reset(0)
    s = JniSampler(jvm, K, V)
    before = standin.fm.fm_log_len()
    for n in (0, M * M, D * M * M):
        raises(ISE, s.sweep, 0, 1, 0, np.ones(n), contains="setCorpus has not been called")
    assert standin.fm.fm_log_len() == before
    s.sweep(0, 1, 0, None)                                    # without view weights the library is asked (and answers for itself)
    assert standin.log()[-1] == "mvhdp_sweep"
    s.close()


def test_a_refused_emb_init_keeps_the_embedding_and_a_failed_one_forgets_it(standin, model):
    n = R * EC
    model.s.embGetVectors(n)
    standin.fm.fm_set_status(-1)                              # MVHDP_ERR_INVALID_ARG: refused before the library touched what it holds
    raises(RTE, model.s.embInit, H.EmbConfig(numColumns=EC + 1, numContextColumns=1), None, 1)
    standin.fm.fm_set_status(0)
    model.s.embGetVectors(n)                                  # the shape is still the old one
    raises(IAE, model.s.embGetVectors, (R) * (EC + 1))
    standin.fm.fm_set_status(-3)                              # any later failure: the library has freed it
    raises(RTE, model.s.embInit, H.EmbConfig(numColumns=EC, numContextColumns=1), None, 1)
    standin.fm.fm_set_status(0)
    before = standin.fm.fm_log_len()
    raises(ISE, model.s.embGetVectors, n, contains="embInit has not been called")
    assert standin.fm.fm_log_len() == before
    model.s.embInit(H.EmbConfig(numColumns=EC, numContextColumns=0, withTopics=False), None, 1)
    model.s.embGetVectors(V[0] * EC)                          # without topics: V_0 rows
    model.s.embSoftmax(True, 0, 0)                            # ... and no topic rows: the arrays of embSoftmax are empty
    raises(IAE, model.s.embSoftmax, True, K * V[0], K)
    model.s.embRelease()
    raises(ISE, model.s.embWordStats, V[0], contains="embInit has not been called")


def test_set_tuning_of_get_tuning_hands_back_every_field(standin, model):
    """setTuning(getTuning()) -- what INTEGRATION.md tells a host to do to carry a learnt walk threshold to a shard -- must not change
    a field, the ones the Java block does not carry (single_wave, learnt_walk_step[3], live_overlap, live_rows) included."""
    t = model.s.getTuning()
    assert (t.forcePrimary, t.narrow, t.walkFixed, t.singleStream, t.live16, t.learntWalkStep, t.primaryMinShare) == (4, 1, 1, 1, 1, [3, 7, 11], 0.375)
    assert t.walkTheta == [0.125 + m for m in range(8)] and t.treeBranchShare == [0.0625 * (m + 1) for m in range(8)]
    model.s.setTuning(t)
    assert standin.fm.fm_tuning_size() == C.sizeof(_lib.TuningC)
    made, given = _lib.TuningC(), _lib.TuningC()
    standin.fm.fm_made_tuning(C.byref(made))
    standin.fm.fm_given_tuning(C.byref(given))
    for name, typ in _lib.TuningC._fields_:
        a, b = getattr(made, name), getattr(given, name)
        a, b = (list(a), list(b)) if hasattr(a, "__len__") else (a, b)
        assert a == b, f"mvhdp_tuning.{name}: the handle held {a}, setTuning(getTuning()) handed the library {b}"
    t.forcePrimary, t.learntWalkStep, t.walkTheta[7] = 8, [1, 2, 5], 0.75      # and what the block does carry arrives
    model.s.setTuning(t)
    standin.fm.fm_given_tuning(C.byref(given))
    assert (given.force_primary, list(given.learnt_walk_step), given.walk_theta[7], given.live_rows) == (8, [1, 2, 5, 13], 0.75, 1)


def test_destroy_twice_destroys_once(standin, jvm):
    standin.reset(0)
    s = JniSampler(jvm, K, V)
    h = s.handle
    jvm.call("nDestroy", h)
    jvm.call("nDestroy", h)
    assert standin.counter("destroys") == 1
    raises(ISE, jvm.call, "nBuildCounts", h)
    before = standin.fm.fm_log_len()
    for name, rest in _handle_argument_calls():               # the jlong of a sampler closed a moment ago: refused by the side entries as well
        if name in H.SIDE_ENTRIES:
            raises(ISE, jvm.call, name, h, *rest, contains="NativeSampler is closed")
    assert standin.fm.fm_log_len() == before
    g = JniGroup(jvm, [JniSampler(jvm, K, V)])
    gh = g.g
    jvm.call("nGroupDestroy", gh); jvm.call("nGroupDestroy", gh)
    assert standin.counter("group_destroys") == 1
    raises(ISE, jvm.call, "nGroupDrain", gh)


def _in_thread(fn, *a):
    box = {}

    def run():
        try:
            box["value"] = fn(*a)
        except BaseException as e:                            # (reported by the test's own thread)
            box["error"] = e
    t = threading.Thread(target=run, daemon=True)
    t.start()
    return t, box


def test_destroy_of_a_member_waits_for_the_group_that_names_it(standin, jvm):
    standin.reset(0)
    a, b = JniSampler(jvm, K, V), JniSampler(jvm, K, V)
    g = JniGroup(jvm, [a, b])
    assert standin.counter("group_n") == 2 and standin.fm.fm_group_member(0) != standin.fm.fm_group_member(1)
    raises(ISE, JniGroup, jvm, [a, closed_sampler(jvm)])        # a closed member: refused, and the pin on `a` it took is given back
    destroyed = standin.counter("destroys")
    t, box = _in_thread(jvm.call, "nDestroy", a.handle)
    try:
        time.sleep(0.3)
        g.buildCounts()                                       # the group still works
        assert t.is_alive() and standin.counter("destroys") == destroyed
        raises(ISE, jvm.call, "nBuildCounts", a.handle)       # ... but nobody finds the member any more
    finally:
        g.close()
        t.join(30)
    assert not t.is_alive() and "error" not in box and standin.counter("destroys") == destroyed + 1
    log = standin.log()
    assert log.index("mvhdp_group_destroy") < len(log) - 1 - log[::-1].index("mvhdp_destroy")
    b.close()
    # the same for a group made of one rank
    c = JniSampler(jvm, K, V)
    g = JniGroup.ofRank(jvm, c, np.zeros(128), 0, 1)
    t, box = _in_thread(jvm.call, "nDestroy", c.handle)
    try:
        time.sleep(0.3)
        assert t.is_alive()
    finally:
        g.close()
        t.join(30)
    assert not t.is_alive() and "error" not in box


def closed_sampler(jvm):
    s = JniSampler(jvm, K, V)
    h = s.handle
    s.close()
    s.handle = h
    return s


def _destroy_waits_for(standin, jvm, s, call, library_name):
    """nDestroy on another thread while call() is held inside the library: it returns only once the call has; returns the call's result"""
    standin.fm.fm_block_sweeps(1)
    inside, sbox = _in_thread(call)
    for _ in range(300):
        if standin.fm.fm_sweeps_inside() == 1:
            break
        time.sleep(0.01)
    if standin.fm.fm_sweeps_inside() != 1:
        standin.fm.fm_block_sweeps(0)
        inside.join(30)
        raise AssertionError(f"{library_name} was not reached: {sbox}")
    closing, cbox = _in_thread(jvm.call, "nDestroy", s.handle)
    try:
        time.sleep(0.3)
        assert closing.is_alive() and standin.counter("destroys") == 0
    finally:
        standin.fm.fm_block_sweeps(0)
        inside.join(30); closing.join(30)
    assert not inside.is_alive() and not closing.is_alive() and "error" not in sbox and "error" not in cbox
    log = standin.log()
    assert standin.fm.fm_sweeps_returned() == 1 and log.index(library_name) < log.index("mvhdp_destroy")
    return sbox["value"]


def test_destroy_waits_for_a_sweep_that_is_inside_the_library(standin, jvm):
    standin.reset(0)
    s = JniSampler(jvm, K, V)
    sts = _destroy_waits_for(standin, jvm, s, lambda: s.sweepMany(0, 2, 1, 0), "mvhdp_sweep_many")
    assert [st.tokens for st in sts] == [1001, 2001]


def test_destroy_waits_for_a_held_out_call_that_is_inside_the_library(standin, jvm):
    """the entries outside mvhdp_jni.cpp pin the handle too: mvhdp_heldout_left_to_right, the longest call the shim makes"""
    standin.reset(0)
    s = JniSampler(jvm, K, V)
    stats = jvm.longs(3)
    args = [s.handle, 0, 3, 1, 17, 0, None, 0.0, jvm.longs([0, 2, 2, 5]), jvm.ints(np.ones(5)), None, None, None, stats]
    assert _destroy_waits_for(standin, jvm, s, lambda: jvm.call("nLeftToRight", *args), "mvhdp_heldout_left_to_right") == -12.5
    assert list(stats.get()) == [301, 302, 303]
    raises(ISE, jvm.call, "nLeftToRight", *args, contains="NativeSampler is closed")


@pytest.mark.parametrize("form", ["four_sources", "one_tu"])
def test_each_build_form_has_one_registry_for_all_four_sources(standin, jvm, form):
    """The four sources on one command line, and one translation unit that includes them: in either, an entry outside mvhdp_jni.cpp
    finds the handle nCreate (inside it) registered, refuses one that was never issued or is closed, and nothing of the shared header
    is exported -- a registry per source would refuse every handle, an exported one could be interposed."""
    j = standin.forms[form]
    standin.reset(0)
    j.lib.fj_ledger_reset(); j.lib.fj_exception_clear()
    for bogus in (0, 0x5a5a5a5a5a58, -8):
        for name, rest in _handle_argument_calls():
            if name not in ("nDestroy", "nGroupDestroy"):
                e = raises(ISE, j.call, name, bogus, *rest)
                assert e.msg in ("NativeSampler is closed", "group is closed"), (name, e.msg)
    assert standin.log() == []
    s = JniSampler(j, K, V)
    s.setCorpus(0, DOC_OFF[0], np.arange(NTOK[0]) % V[0])
    h, stats = s.handle, j.longs(5)
    good = {"nSimilarPairs": [h, 1, SN, SD, j.doubles(SN * SD), 0.03, 0.15, 0, 0, j.ints(CAP), j.ints(CAP), j.doubles(CAP), stats, None],
            "nDocTopicsTop": [h, j.doubles(M), 0, D, 0.03, 3, None, j.ints(CAP), j.doubles(CAP)],
            "nEntityTopicDistributions": [h, j.doubles(M), 0.03, -1, 5, j.longs([0, 1]), j.longs([0]), j.doubles(K)],
            "nTopicPhrases": [h, 20, 0, None, None, None, None, None, None, j.longs(2), None],
            "nLeftToRight": [h, 0, 3, 1, 17, 0, None, 0.0, j.longs([0, 2]), j.ints([1, 2]), None, None, None, None]}
    assert sorted(good) == sorted(H.SIDE_ENTRIES)
    want = {"nSimilarPairs": 3, "nDocTopicsTop": 2, "nEntityTopicDistributions": None, "nTopicPhrases": 0, "nLeftToRight": -12.5}
    for name, args in good.items():
        assert j.call(name, *args) == want[name], name
    assert list(stats.get()) == [101, 102, 103, 104, 105]
    assert standin.log()[-5:] == ["mvhdp_similar_pairs", "mvhdp_doc_topics_top", "mvhdp_entity_topic_distributions", "mvhdp_topic_phrases",
                                  "mvhdp_heldout_left_to_right"]
    s.close()
    for name, args in good.items():
        raises(ISE, j.call, name, *args, contains="NativeSampler is closed")
    exported = subprocess.check_output(["nm", "-D", "--defined-only", j.path], text=True).split("\n")
    names = [line.split()[-1] for line in exported if line.strip()]
    assert sum(n.startswith("Java_") for n in names) == 56
    leaked = [n for n in names if "mvhdp_jni" in n or re.search(r"g_reg|g_shards|g_groups|throw_|bad_len|Pin|4Ints|5Longs|7Doubles", n)]
    assert not leaked, leaked


def test_a_failing_get_elements_leaves_the_library_uncalled_and_nothing_held(standin, model):
    tried = 0
    for name in GOOD:
        model.jvm.call(name, *model.args(name))
        gets = model.jvm.last_ledger["elements_gets"]
        for nth in range(1, gets + 1):
            args = model.args(name)
            before = standin.fm.fm_log_len()
            model.jvm.fail_elements_at(nth)
            e = raises(OOM, model.jvm.call, name, *args)      # (call() has checked that every buffer taken before was released)
            model.jvm.fail_elements_at(0)
            assert standin.fm.fm_log_len() == before, f"{name}: {standin.log()[before:]} called after Get<Type>ArrayElements {nth} of {gets} failed"
            tried += 1
    assert tried >= 60, tried


def test_every_entry_is_executed(standin, model):
    """all 56, each through to the library and back (the stand-in answers MVHDP_OK)"""
    jvm = model.jvm
    jvm.log.clear()
    before = standin.fm.fm_log_len()
    for name in GOOD:
        jvm.call(name, *model.args(name))
    for name in NO_ARRAYS["h"]:
        jvm.call(name, model.s.handle)
    for name in NO_ARRAYS["g"]:
        jvm.call(name, model.group.g)
    jvm.call("nApplyDelta", model.s.handle, 2, 1)
    jvm.call("nEmbRelease", model.s.handle)
    s2 = JniSampler(jvm, K, V)                                # nCreate
    g2 = JniGroup(jvm, [s2])                                  # nGroupCreate
    g3 = JniGroup.ofRank(jvm, model.s, np.zeros(128), 0, 1)   # nGroupCreateRank
    g3.close(); g2.close(); s2.close()                        # nGroupDestroy, nDestroy
    assert sorted(set(jvm.log)) == sorted(H.shim_signatures()) and len(set(jvm.log)) == 56
    called = set(standin.log()[before:])
    imports, _ = H.shim_imports(model.tmp)
    assert called == imports - {"mvhdp_last_error", "mvhdp_group_last_error"}      # every mvhdp_* the shim imports but the two messages
