"""Runs the JNI shim (the four sources mvtopicmodel_amd/java/mvhdp*_jni.cpp, one libmvhdp_jni.so) without a JVM.

The sources are compiled UNMODIFIED against the declaration-only tests/native/jni_stub/jni.h and linked, in a temporary directory, with
tests/native/fake_jvm.cpp (which defines the JNIEnv members that header declares) and with either libmvhdp.so or the CPU-side stand-in
tests/native/fake_mvhdp.c -- in either of the two forms a host may build them: the four on one command line, or one translation unit
that includes all four.  `Jvm` is what a test holds: arrays and objects of the fake Java heap, `call()` for one Java_..._n* entry of any
of the four classes.
After EVERY entry `call()` reads the ledger of the fake JVM and refuses a dirty one -- on the error paths too -- and turns a pending
exception into a Python `JavaException(cls, msg)`.  `JniSampler` / `JniGroup` transcribe the public methods of NativeSampler.java
line by line: the same array lengths, the same flat layouts, the same way of filling SweepStats / EmbStats / Tuning / Diagnostics.

Test infrastructure; nothing here is part of the product or of its build."""
import ctypes as C
import functools
import os
import re
import subprocess
import tempfile
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JAVA_DIR = os.path.join(ROOT, "mvtopicmodel_amd", "java")
# the Java classes and the shim source that holds the natives of each (mvhdp_jni.cpp first: SHIM)
CLASSES = {"NativeSampler": "mvhdp_jni.cpp", "NativeSimilarity": "mvhdp_sim_jni.cpp", "NativePhrases": "mvhdp_phrases_jni.cpp", "NativeHeldout": "mvhdp_heldout_jni.cpp"}
SHIMS = [os.path.join(JAVA_DIR, f) for f in CLASSES.values()]
# MVHDP_JNI_SHIM_SOURCE: a scratch copy of ONE of the four sources with one mutation applied (profiles/jni_harness.md) takes the place of
# the source of the same base name (its #include "mvhdp_jni_common.h" finds a header lying beside the copy first, the repository's
# otherwise).  Said aloud on import (pytest lists the warning in its summary), so that a stray value cannot pass for a run against the
# repository's own files.
if os.environ.get("MVHDP_JNI_SHIM_SOURCE"):
    _copy = os.path.abspath(os.environ["MVHDP_JNI_SHIM_SOURCE"])
    if not os.path.isfile(_copy) or os.path.basename(_copy) not in CLASSES.values():
        raise RuntimeError(f"MVHDP_JNI_SHIM_SOURCE={_copy}: not a file named as one of {sorted(CLASSES.values())}")
    SHIMS[list(CLASSES.values()).index(os.path.basename(_copy))] = _copy
    warnings.warn(f"MVHDP_JNI_SHIM_SOURCE is set: the JNI tests run {_copy}, NOT mvtopicmodel_amd/java/{os.path.basename(_copy)}", RuntimeWarning)
SHIM = SHIMS[0]
COMMON = os.path.join(JAVA_DIR, "mvhdp_jni_common.h")        # what the four sources share
JAVA = {cls: os.path.join(JAVA_DIR, "org", "madgik", "MVTopicModel", cls + ".java") for cls in CLASSES}
NATIVE = os.path.join(ROOT, "tests", "native")
PREFIX = {cls: f"Java_org_madgik_MVTopicModel_{cls}_" for cls in CLASSES}
JNI_ABORT = 2

# ---- the 56 entries, by class: return type, then the arguments after (JNIEnv*, jclass).  J jlong, I jint, D jdouble, Z jboolean, V void;
# [I int[], [J long[], [D double[], [Z boolean[], [B byte[], [[D double[][], L an object ----
DIAG = ["I", "[I", "[D", "[D", "[I", "[I", "[I", "[I", "[I", "[I", "[I", "[D", "[I", "[J", "[D"]
_BY_CLASS = {"NativeSampler": {
    "nCreate": ("J", ["I", "[I", "I", "J"]),
    "nDestroy": ("V", ["J"]),
    "nSetCorpus": ("V", ["J", "I", "[J", "[I"]),
    "nSetAssignments": ("V", ["J", "I", "[I"]),
    "nSetViewPresence": ("V", ["J", "I", "[Z"]),
    "nGetAssignments": ("V", ["J", "I", "[I"]),
    "nSetHyper": ("V", ["J", "[[D", "[D", "[D", "[D", "[D", "[[D", "[[D", "[Z"]),
    "nBuildCounts": ("V", ["J"]),
    "nBuildTrees": ("V", ["J"]),
    "nGetCounts": ("V", ["J", "I", "[I", "[I"]),
    "nGetDocTopicHist": ("V", ["J", "I", "[I", "I", "[I"]),
    "nGetAlpha": ("V", ["J", "[D", "[Z"]),
    "nSweep": ("V", ["J", "I", "J", "I", "[D", "L"]),
    "nApplyDelta": ("V", ["J", "I", "I"]),
    "nModelLogLikelihood": ("V", ["J", "[D"]),
    "nSweepMany": ("V", ["J", "I", "I", "J", "I", "[J"]),
    "nGetTuning": ("V", ["J", "[I", "[D"]),
    "nSetTuning": ("V", ["J", "[I", "[D"]),
    "nGroupCreate": ("J", ["[J"]),
    "nGroupUniqueId": ("V", ["[B"]),
    "nGroupCreateRank": ("J", ["J", "[B", "I", "I"]),
    "nGroupDestroy": ("V", ["J"]),
    "nGroupBuildCounts": ("V", ["J"]),
    "nGroupSweep": ("D", ["J", "I", "J", "I", "[J", "[I"]),
    "nGetCountHistogram": ("V", ["J", "I", "[I"]),
    "nViewOverlapSums": ("V", ["J", "[D"]),
    "nGammaDocStatistics": ("V", ["J", "I", "D", "J", "I", "[D"]),
    "nDpTableStatistics": ("V", ["J", "I", "[I", "I", "[D", "J", "I", "[D", "[B"]),
    "nGroupDrain": ("V", ["J"]),
    "nGroupAbort": ("V", ["J"]),
    "nGroupModelLogLikelihood": ("V", ["J", "[D"]),
    "nGroupGetDocTopicHist": ("V", ["J", "I", "[I", "I", "[I"]),
    "nGroupGetCountHistogram": ("V", ["J", "I", "[I"]),
    "nGroupViewOverlapSums": ("V", ["J", "[D"]),
    "nGroupGammaDocStatistics": ("V", ["J", "I", "D", "J", "I", "[D"]),
    "nTopWords": ("V", ["J", "I", "I", "[I", "[I", "[I"]),
    "nDiscrWeights": ("V", ["J", "[D", "I", "[D"]),
    "nDiagnostics": ("V", ["J"] + DIAG),
    "nGroupDiagnostics": ("V", ["J"] + DIAG),
    "nEmbInit": ("V", ["J", "[I", "J", "[D", "[D", "J"]),
    "nEmbCountWords": ("V", ["J"]),
    "nEmbTrain": ("V", ["J", "I", "J", "I", "I", "[J", "[D"]),
    "nEmbGetVectors": ("V", ["J", "[D", "[D"]),
    "nEmbSetVectors": ("V", ["J", "[D", "[D"]),
    "nEmbWordStats": ("V", ["J", "[J", "[D", "[J"]),
    "nEmbSamplingTable": ("V", ["J", "J", "[I"]),
    "nEmbSoftmax": ("V", ["J", "Z", "[D", "[D"]),
    "nEmbNearest": ("V", ["J", "[D", "I", "[I", "[D", "[I", "[D"]),
    "nEmbRelease": ("V", ["J"]),
    "nSetVectorsMix": ("V", ["J", "D", "[D", "[D"]),
    "nGetVectorsMix": ("D", ["J", "[D"]),
}, "NativeSimilarity": {
    "nSimilarPairs": ("J", ["J", "I", "I", "I", "[D", "D", "D", "I", "J", "[I", "[I", "[D", "[J", "[D"]),
    "nDocTopicsTop": ("J", ["J", "[D", "J", "J", "D", "I", "[J", "[I", "[D"]),
    "nEntityTopicDistributions": ("V", ["J", "[D", "D", "I", "I", "[J", "[J", "[D"]),
}, "NativePhrases": {
    "nTopicPhrases": ("J", ["J", "I", "I", "[J", "[J", "[I", "[I", "[J", "[J", "[J", "[J"]),
}, "NativeHeldout": {
    "nLeftToRight": ("D", ["J", "I", "I", "I", "J", "J", "[D", "D", "[J", "[I", "[D", "[D", "[J", "[J"]),
}}
# {entry: (return code, [argument codes], Java class)}: the entry names are unique across the four classes
PROTOTYPES = {name: (ret, args, cls) for cls, table in _BY_CLASS.items() for name, (ret, args) in table.items()}
SIDE_ENTRIES = [name for name, (_, _, cls) in PROTOTYPES.items() if cls != "NativeSampler"]
_CTYPE = {"J": C.c_int64, "I": C.c_int32, "D": C.c_double, "Z": C.c_uint8, "V": None}
_CXX = {"jlong": "J", "jint": "I", "jdouble": "D", "jboolean": "Z", "void": "V", "jintArray": "[I", "jlongArray": "[J", "jdoubleArray": "[D",
        "jbooleanArray": "[Z", "jbyteArray": "[B", "jobjectArray": "[[D", "jobject": "L"}
_KIND = {"[I": "I", "[J": "J", "[D": "D", "[Z": "Z", "[B": "B", "[[D": "L"}
_DTYPE = {"I": np.int32, "J": np.int64, "D": np.float64, "Z": np.uint8, "B": np.int8}

LEDGER = ["buffers_outstanding", "bad_releases", "guard_damage", "locals_left", "local_arrays_left", "locals_high_water", "region_oob",
          "calls_while_pending", "misuse", "elements_gets", "jni_calls"]
# what must be zero after every entry; locals_left counts the class references of FindClass / GetObjectClass too, which a JVM frees when
# the native method returns, so only the array references an entry left behind and the high-water mark (16 guaranteed) are held against it
DIRTY = ["buffers_outstanding", "bad_releases", "guard_damage", "local_arrays_left", "region_oob", "calls_while_pending", "misuse"]
LOCAL_CAPACITY = 16

SWEEP_STATS_FIELDS = "tokens:J,changed:J,newMassCnt:J,topicDocMassCnt:J,wordFTreeMassCnt:J,oovSkipped:J,abortedDocs:J,exactFallbacks:J," \
                     "activatedTopic:I,activatedModality:I,activationKey:J,sweepKernelMs:D,totalMs:D,activations:I"
SWEEP_STATS_CLASS = "org/madgik/MVTopicModel/NativeSampler$SweepStats"


class JavaException(Exception):
    def __init__(self, cls, msg):
        super().__init__(f"{cls}: {msg}")
        self.cls, self.msg = cls, msg


class DirtyLedger(AssertionError):
    pass


def shim_signatures(paths=None):
    """{entry: (return code, [argument codes], Java class)} parsed from the four shim sources (the DIAG_PARAMS macro expanded)."""
    out = {}
    for path in paths or SHIMS:
        src = open(path).read()
        macro = re.search(r"#define DIAG_PARAMS (.*?[^\\])\n", src, re.S)
        macro = macro.group(1).replace("\\\n", " ") if macro else ""
        for ret, cls, name, params in re.findall(r"JNIEXPORT (\w+) JNICALL Java_org_madgik_MVTopicModel_([A-Za-z]+)_(n\w+)\(([^)]*)\)\s*\{", src):
            params = params.replace("DIAG_PARAMS", macro)
            parts = [p.strip() for p in params.split(",")]
            assert parts[0].startswith("JNIEnv*") and parts[1].split()[0] == "jclass", (name, parts[:2])
            assert name not in out and os.path.basename(path) == CLASSES[cls], (name, cls, path)
            out[name] = (_CXX[ret], [_CXX[p.split()[0]] for p in parts[2:]], cls)
    return out


def java_natives():
    """{native method: (return code, [argument codes], Java class)} parsed from the `private static native` lines of the four Java classes."""
    jt = {"long": "J", "int": "I", "double": "D", "boolean": "Z", "void": "V", "int[]": "[I", "long[]": "[J", "double[]": "[D", "boolean[]": "[Z",
          "byte[]": "[B", "double[][]": "[[D", "SweepStats": "L"}
    out = {}
    for cls, path in JAVA.items():
        for ret, name, params in re.findall(r"private static native ([\w\[\]]+) (n\w+)\(([^)]*)\);", open(path).read()):
            assert name not in out, name
            out[name] = (jt[ret], [jt[p.split()[0]] for p in params.split(",")], cls)
    return out


def build_standin(tmp):
    """tests/native/fake_mvhdp.c as libfake_mvhdp.so in `tmp`; returns its path."""
    out = os.path.join(str(tmp), "libfake_mvhdp.so")
    subprocess.check_call(["gcc", "-O1", "-g", "-shared", "-fPIC", "-fvisibility=hidden", "-I", os.path.join(ROOT, "include"),
                           os.path.join(NATIVE, "fake_mvhdp.c"), "-o", out, "-pthread"])
    return out


_INCLUDES = ["-I", os.path.join(NATIVE, "jni_stub"), "-I", os.path.join(ROOT, "include"), "-I", JAVA_DIR]


def build_shim(tmp, library, shims=None, name="libmvhdp_jni_under_test.so", one_tu=False):
    """the shim sources + fake JVM as one shared object in `tmp`, linked against `library` (libmvhdp.so or the stand-in); returns its
    path.  one_tu: the sources as one translation unit that includes them all, instead of each on the command line."""
    out = os.path.join(str(tmp), name)
    libdir, base = os.path.split(os.path.abspath(library))
    assert base.startswith("lib") and base.endswith(".so"), base
    shims = list(shims or SHIMS)
    if one_tu:
        tu = os.path.join(str(tmp), name + ".one_tu.cpp")
        with open(tu, "w") as f:
            f.write("".join(f'#include "{s}"\n' for s in shims))
        shims = [tu]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-shared", "-fPIC", "-Wall"] + _INCLUDES + shims + [os.path.join(NATIVE, "fake_jvm.cpp"), "-o", out,
                           "-Wl,-Bsymbolic", "-Wl,--no-undefined", "-L", libdir, "-l" + base[3:-3], "-Wl,-rpath," + libdir, "-pthread"])
    return out


def shim_imports(tmp, shims=None):
    """the mvhdp_* symbols the shim sources' object files leave undefined (nm -u), and the JNIEnv members"""
    names = set()
    for i, shim in enumerate(shims or SHIMS):
        obj = os.path.join(str(tmp), f"shim_only_{i}.o")
        subprocess.check_call(["g++", "-std=c++17", "-c", "-fPIC"] + _INCLUDES + [shim, "-o", obj])
        names |= set(subprocess.check_output(["nm", "-u", obj], text=True).split())
    return {n for n in names if n.startswith("mvhdp_")}, {n for n in names if n.startswith("_ZN6JNIEnv")}


@functools.lru_cache(maxsize=None)
def check_sources_compile_together_and_apart():
    """What a namespace per source once stood for: each of the four sources type-checks on its own (-Wall -Werror), all four type-check
    as one translation unit, and neither they nor the shared header contain a using-directive (a `using namespace` in one source
    would change name lookup in the ones included after it).  Nothing is built or linked; once per process."""
    for shim in SHIMS:
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror"] + _INCLUDES + [shim])
    with tempfile.TemporaryDirectory() as tmp:
        tu = os.path.join(tmp, "one_tu.cpp")
        with open(tu, "w") as f:
            f.write("".join(f'#include "{s}"\n' for s in SHIMS))
        subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror"] + _INCLUDES + [tu])
    for path in SHIMS + [COMMON]:
        assert not re.search(r"using\s+namespace", re.sub(r"//[^\n]*", "", open(path).read())), path
    return True


def common_header_code():
    """mvhdp_jni_common.h without its comments"""
    return re.sub(r"//[^\n]*", "", open(COMMON).read())


class JArray:
    """an array on the fake Java heap"""

    def __init__(self, jvm, kind, h, keep=None):
        self.jvm, self.kind, self.h, self.keep = jvm, kind, h, keep

    def __len__(self):
        return self.jvm.lib.fj_array_length(self.h)

    def get(self):
        n = len(self)
        out = np.zeros(n, dtype=_DTYPE[self.kind])
        if n:
            C.memmove(out.ctypes.data, self.jvm.lib.fj_array_data(self.h), out.nbytes)
        return out

    def put(self, values):
        v = np.ascontiguousarray(values, dtype=_DTYPE[self.kind]).ravel()
        assert len(v) == len(self)
        if len(v):
            C.memmove(self.jvm.lib.fj_array_data(self.h), v.ctypes.data, v.nbytes)

    def __del__(self):
        try:
            self.jvm.lib.fj_free(self.h)
        except Exception:
            pass


class JObject:
    def __init__(self, jvm, h, fields):
        self.jvm, self.h, self.fields = jvm, h, fields

    def get(self, name):
        sig = dict(f.split(":") for f in self.fields.split(","))[name]
        if sig == "D":
            return self.jvm.lib.fj_get_double_field(self.h, name.encode())
        return self.jvm.lib.fj_get_integral_field(self.h, name.encode())

    def __del__(self):
        try:
            self.jvm.lib.fj_free(self.h)
        except Exception:
            pass


class Jvm:
    """One loaded (shim + fake JVM) library."""

    def __init__(self, path):
        self.path = path
        self.lib = L = C.CDLL(path)
        vp = C.c_void_p
        L.fj_env.restype = vp
        L.fj_new_array.restype = vp; L.fj_new_array.argtypes = [C.c_char, C.c_int32]
        L.fj_array_length.restype = C.c_int32; L.fj_array_length.argtypes = [vp]
        L.fj_array_data.restype = vp; L.fj_array_data.argtypes = [vp]
        L.fj_set_object_element.argtypes = [vp, C.c_int32, vp]
        L.fj_new_object.restype = vp; L.fj_new_object.argtypes = [C.c_char_p, C.c_char_p]
        L.fj_has_field.argtypes = [vp, C.c_char_p]
        L.fj_get_integral_field.restype = C.c_int64; L.fj_get_integral_field.argtypes = [vp, C.c_char_p]
        L.fj_get_double_field.restype = C.c_double; L.fj_get_double_field.argtypes = [vp, C.c_char_p]
        L.fj_free.argtypes = [vp]
        L.fj_live_objects.restype = C.c_int64
        L.fj_exception.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
        L.fj_ledger.argtypes = [C.POINTER(C.c_int64)]
        L.fj_fail_elements_at.argtypes = [C.c_int64]
        L.fj_test_get_elements.restype = vp; L.fj_test_get_elements.argtypes = [vp]
        L.fj_test_release_elements.argtypes = [vp, vp, C.c_int32]
        L.fj_test_get_int_region.argtypes = [vp, C.c_int32, C.c_int32, vp]
        L.fj_test_set_int_region.argtypes = [vp, C.c_int32, C.c_int32, vp]
        L.fj_test_array_length.argtypes = [vp]; L.fj_test_array_length.restype = C.c_int32
        L.fj_test_object_element.restype = vp; L.fj_test_object_element.argtypes = [vp, C.c_int32]
        L.fj_test_delete_local.argtypes = [vp]
        L.fj_test_find_class.argtypes = [C.c_char_p]
        L.fj_test_throw.argtypes = [C.c_char_p, C.c_char_p]
        L.fj_test_set_long_field.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_int64]
        assert L.fj_ledger_size() == len(LEDGER)
        self.env = L.fj_env()
        self.entries = {}
        for name, (ret, args, cls) in PROTOTYPES.items():
            f = getattr(L, PREFIX[cls] + name)
            f.restype = _CTYPE[ret]
            f.argtypes = [vp, vp] + [_CTYPE.get(a, vp) for a in args]
            self.entries[name] = f
        self.log = []                                         # every entry called through call(), in order
        self.last_ledger = None

    # ---- the fake Java heap ----
    def array(self, kind, values):
        """int[] / long[] / double[] / boolean[] / byte[] ('I' 'J' 'D' 'Z' 'B') holding `values`, or of that many zeros"""
        if isinstance(values, (int, np.integer)):
            values = np.zeros(int(values), dtype=_DTYPE[kind])
        v = np.ascontiguousarray(values, dtype=_DTYPE[kind]).ravel()
        a = JArray(self, kind, self.lib.fj_new_array(kind.encode(), len(v)))
        a.put(v)
        return a

    def ints(self, v): return self.array("I", v)
    def longs(self, v): return self.array("J", v)
    def doubles(self, v): return self.array("D", v)
    def booleans(self, v): return self.array("Z", v)
    def bytes(self, v): return self.array("B", v)

    def rows(self, matrix):
        """double[][]: an Object[] of double[] rows (a row may be None)"""
        rows = [None if r is None else self.doubles(r) for r in matrix]
        a = JArray(self, "L", self.lib.fj_new_array(b"L", len(rows)), keep=rows)
        for i, r in enumerate(rows):
            self.lib.fj_set_object_element(a.h, i, None if r is None else r.h)
        return a

    def object(self, cls, fields):
        h = self.lib.fj_new_object(cls.encode(), fields.encode())
        assert h, f"class {cls} was declared with other fields"
        return JObject(self, h, fields)

    # ---- the ledger and the pending exception ----
    def ledger(self):
        buf = (C.c_int64 * len(LEDGER))()
        self.lib.fj_ledger(buf)
        return dict(zip(LEDGER, buf))

    def pending(self):
        c, m = C.c_char_p(), C.c_char_p()
        if not self.lib.fj_exception(C.byref(c), C.byref(m)):
            return None
        return c.value.decode(), m.value.decode()

    def take_exception(self):
        p = self.pending()
        self.lib.fj_exception_clear()
        return p

    def dirt(self, led=None):
        led = led or self.ledger()
        bad = {k: led[k] for k in DIRTY if led[k]}
        if led["locals_high_water"] > LOCAL_CAPACITY:
            bad["locals_high_water"] = led["locals_high_water"]
        return bad

    def call(self, name, *args):
        """One Java_..._n* entry as the JVM would call it: a fresh local frame, the entry, the frame popped; then the ledger must be
        clean (DirtyLedger if not, whatever else happened) and a pending exception is raised as JavaException."""
        ret, codes, _ = PROTOTYPES[name]
        assert len(args) == len(codes), f"{name} takes {len(codes)} arguments"
        conv = []
        for a, code in zip(args, codes):
            if code in _KIND:
                assert a is None or (isinstance(a, JArray) and a.kind == _KIND[code]), f"{name}: {code} expected, got {a!r}"
                conv.append(None if a is None else a.h)
            elif code == "L":
                conv.append(None if a is None else a.h)
            elif code == "D":
                conv.append(float(a))
            else:
                conv.append(int(a))
        self.log.append(name)
        before = self.ledger()
        self.lib.fj_begin_call()
        r = self.entries[name](self.env, None, *conv)
        self.lib.fj_end_call()
        led = self.ledger()
        self.last_ledger = {k: (led[k] if k in ("buffers_outstanding", "locals_left", "local_arrays_left", "locals_high_water") else led[k] - before[k]) for k in LEDGER}
        exc = self.take_exception()
        bad = self.dirt(self.last_ledger)
        if bad:
            self.lib.fj_ledger_reset()
            raise DirtyLedger(f"{name}: the fake JVM's ledger is not clean: {bad}" + (f" (pending: {exc[0]}: {exc[1]})" if exc else ""))
        if exc:
            raise JavaException(*exc)
        return r

    def fail_elements_at(self, n):
        self.lib.fj_fail_elements_at(int(n))


# ---------------------------------------------------------------------------------------------------------------------------------
# NativeSampler.java, transcribed: one method here per public method there, the same arrays of the same lengths in the same order.
def _stats_from_flat(flat, i):                                # NativeSampler.statsFromFlat
    st = types.SimpleNamespace(tokens=0, changed=0, newMassCnt=0, topicDocMassCnt=0, wordFTreeMassCnt=0, oovSkipped=0, abortedDocs=0, exactFallbacks=0,
                               activatedTopic=0, activatedModality=0, activationKey=0, sweepKernelMs=0.0, totalMs=0.0, activations=0)
    (st.tokens, st.changed, st.newMassCnt, st.topicDocMassCnt, st.wordFTreeMassCnt, st.oovSkipped, st.abortedDocs, st.exactFallbacks) = \
        (int(x) for x in flat[8 * i:8 * i + 8])
    return st


class Tuning:                                                 # NativeSampler.Tuning, with its initial values
    def __init__(self):
        self.forcePrimary, self.narrow, self.walkFixed, self.singleStream, self.live16 = 0, -1, 0, 0, -1
        self.learntWalkStep = [-1, -1, -1]
        self.primaryMinShare = 0.0
        self.walkTheta, self.treeBranchShare = [0.0] * 8, [0.0] * 8


class EmbConfig:                                              # NativeSampler.EmbConfig, with its initial values
    def __init__(self, **kw):
        self.numColumns, self.numContextColumns, self.window, self.numSamples, self.minDocLength, self.sigmoidCacheSize = 200, 50, 5, 5, 10, 1000
        self.withTopics = True
        self.samplingTableSize = 100000000
        self.samplingFactor, self.minExp, self.maxExp = 1e-4, -6.0, 6.0
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


class JniDiagnostics:                                         # NativeSampler.Diagnostics
    ROWS = ["tokens", "document_entropy", "word-length", "coherence", "normDiscrWeight", "discrWeight", "uniform_dist", "corpus_dist", "eff_num_words",
            "token-doc-diff", "rank_1_docs", "allocation_ratio", "allocation_count"]

    def __init__(self, jvm, K, N, V0, M):
        R = len(self.ROWS)
        self.numTopics, self.numTopWords = K, N
        self.scores, self.wordScores, self.sumCountLogCount = jvm.doubles(R * K), jvm.doubles(R * K * N), jvm.doubles(K)
        self.discrWeightPerModality, self.codoc, self.topTypes, self.topCounts = jvm.doubles(M), jvm.ints(K * N * N), jvm.ints(K * N), jvm.ints(K * N)
        self.nonzero, self.numRank1Documents, self.numNonZeroDocuments, self.numDocumentsAtProportions = jvm.ints(K), jvm.ints(K), jvm.ints(K), jvm.ints(K * 7)
        self.wordTypeCounts = jvm.ints(V0)
        self.numTokens = jvm.longs(1)

    def arrays(self):                                         # in the order nDiagnostics / nGroupDiagnostics take them
        return (self.scores, self.wordScores, self.codoc, self.topTypes, self.topCounts, self.nonzero, self.numRank1Documents, self.numNonZeroDocuments,
                self.numDocumentsAtProportions, self.sumCountLogCount, self.wordTypeCounts, self.numTokens, self.discrWeightPerModality)


class JniSampler:
    SWEEP_NO_APPLY, SWEEP_LIVE, EMB_SERIAL = 0x2, 0x20, 0x1

    @staticmethod
    def sweepLiveSegments(n):
        return (n & 0xff) << 16

    def __init__(self, jvm, numTopics, numTypes, device=0, docIdBase=0):
        self.jvm = jvm
        self.handle = 0
        self.handle = jvm.call("nCreate", numTopics, jvm.ints(numTypes), device, docIdBase)

    def call(self, name, *args):
        return self.jvm.call(name, self.handle, *args)

    def setCorpus(self, m, docOff, tokens):
        self.call("nSetCorpus", m, self.jvm.longs(docOff), self.jvm.ints(tokens))

    def setAssignments(self, m, z):
        self.call("nSetAssignments", m, self.jvm.ints(z))

    def getAssignments(self, m, n):
        z = self.jvm.ints(n)
        self.call("nGetAssignments", m, z)
        return z.get()

    def setViewPresence(self, m, present):
        self.call("nSetViewPresence", m, None if present is None else self.jvm.booleans(present))

    def setHyper(self, alpha, alphaSum, beta, betaSum, gamma, p_a, p_b, inactive):
        j = self.jvm
        self.call("nSetHyper", j.rows(alpha), j.doubles(alphaSum), j.doubles(beta), j.doubles(betaSum), j.doubles(gamma), j.rows(p_a), j.rows(p_b),
                  None if inactive is None else j.booleans(inactive))

    def buildCounts(self):
        self.call("nBuildCounts")

    def buildTrees(self):
        self.call("nBuildTrees")

    def getCounts(self, m, V, K):
        nwk, nk = self.jvm.ints(V * K), self.jvm.ints(K)
        self.call("nGetCounts", m, nwk, nk)
        return nwk.get().reshape(V, K), nk.get()

    def getDocTopicHist(self, m, K, histLen, lensLen=0):
        hist, lens = self.jvm.ints(K * histLen), (self.jvm.ints(lensLen) if lensLen else None)
        self.call("nGetDocTopicHist", m, hist, histLen, lens)
        return hist.get().reshape(K, histLen), (lens.get() if lens else None)

    def getAlpha(self, M, K):
        a, ina = self.jvm.doubles(M * (K + 1)), self.jvm.booleans(K)
        self.call("nGetAlpha", a, ina)
        return a.get().reshape(M, K + 1), ina.get()

    def sweep(self, sweepIdx, seed, flags, pOverride=None):
        st = self.jvm.object(SWEEP_STATS_CLASS, SWEEP_STATS_FIELDS)                      # new SweepStats()
        self.call("nSweep", sweepIdx, seed, flags, None if pOverride is None else self.jvm.doubles(pOverride), st)
        return types.SimpleNamespace(**{f.split(":")[0]: st.get(f.split(":")[0]) for f in SWEEP_STATS_FIELDS.split(",")})

    def applyDelta(self, activatedTopic, activatedModality):
        self.call("nApplyDelta", activatedTopic, activatedModality)

    def modelLogLikelihood(self, numModalities):
        ll = self.jvm.doubles(numModalities)
        self.call("nModelLogLikelihood", ll)
        return ll.get()

    def getCountHistogram(self, m, length):
        h = self.jvm.ints(length)
        self.call("nGetCountHistogram", m, h)
        return h.get()

    def viewOverlapSums(self, numModalities):
        s = self.jvm.doubles(numModalities * numModalities)
        self.call("nViewOverlapSums", s)
        return s.get()

    def gammaDocStatistics(self, m, gammaM, seed, round_):
        o = self.jvm.doubles(2)
        self.call("nGammaDocStatistics", m, gammaM, seed, round_, o)
        return o.get()

    def dpTableStatistics(self, m, hist, histLen, conc, seed, round_, K):
        mk, active = self.jvm.doubles(K), self.jvm.bytes(K)
        self.call("nDpTableStatistics", m, self.jvm.ints(hist), histLen, self.jvm.doubles(conc), seed, round_, mk, active)
        return mk.get(), active.get()

    def sweepMany(self, firstIdx, n, seed, flags):
        flat = self.jvm.longs(n * 8)
        self.call("nSweepMany", firstIdx, n, seed, flags, flat)
        f = flat.get()
        return [_stats_from_flat(f, i) for i in range(n)]

    def embInit(self, c, weightsFlat, seed):
        ints = [c.numColumns, c.numContextColumns, 1 if c.withTopics else 0, c.window, c.numSamples, c.minDocLength, c.sigmoidCacheSize]
        self.call("nEmbInit", self.jvm.ints(ints), c.samplingTableSize, self.jvm.doubles([c.samplingFactor, c.minExp, c.maxExp]),
                  None if weightsFlat is None else self.jvm.doubles(weightsFlat), seed)

    def embCountWords(self):
        self.call("nEmbCountWords")

    def embTrain(self, epochs, seed, round_, flags):
        l, d = self.jvm.longs(7), self.jvm.doubles(3)
        self.call("nEmbTrain", epochs, seed, round_, flags, l, d)
        l, d = l.get(), d.get()
        return types.SimpleNamespace(wordsSoFar=int(l[0]), wordsSampled=int(l[1]), wordsConsidered=int(l[2]), docsSkipped=int(l[3]), calls=int(l[4]),
                                     negativesSkipped=int(l[5]), lastEpochCalls=int(l[6]), residual=d[0], lastEpochResidual=d[1], kernelMs=d[2])

    def embGetVectors(self, n, want_weights=True, want_negative=True):
        w, g = (self.jvm.doubles(n) if want_weights else None), (self.jvm.doubles(n) if want_negative else None)
        self.call("nEmbGetVectors", w, g)
        return (w.get() if w else None), (g.get() if g else None)

    def embSetVectors(self, weightsFlat, negativeWeightsFlat):
        self.call("nEmbSetVectors", None if weightsFlat is None else self.jvm.doubles(weightsFlat),
                  None if negativeWeightsFlat is None else self.jvm.doubles(negativeWeightsFlat))

    def embWordStats(self, V0, want_counts=True, want_retention=True):
        c, r, t = (self.jvm.longs(V0) if want_counts else None), (self.jvm.doubles(V0) if want_retention else None), self.jvm.longs(1)
        self.call("nEmbWordStats", c, r, t)
        return (c.get() if c else None), (r.get() if r else None), int(t.get()[0])

    def embSamplingTable(self, first, n):
        t = self.jvm.ints(n)
        self.call("nEmbSamplingTable", first, t)
        return t.get()

    def embSoftmax(self, resetSums, expLen, sumLen):
        e, s = (None if expLen is None else self.jvm.doubles(expLen)), (None if sumLen is None else self.jvm.doubles(sumLen))
        self.call("nEmbSoftmax", 1 if resetSums else 0, e, s)
        return (None if e is None else e.get()), (None if s is None else s.get())

    def embNearest(self, query, n, want_topics=True):
        j = self.jvm
        words, wordSims = j.ints(n), j.doubles(n)
        topics, topicSims = (j.ints(n), j.doubles(n)) if want_topics else (None, None)
        self.call("nEmbNearest", j.doubles(query), n, words, wordSims, topics, topicSims)
        return words.get(), wordSims.get(), (topics.get() if topics else None), (topicSims.get() if topicSims else None)

    def embRelease(self):
        self.call("nEmbRelease")

    def setVectorsMix(self, lam, expDotFlat, sumExp):
        self.call("nSetVectorsMix", lam, None if expDotFlat is None else self.jvm.doubles(expDotFlat), None if sumExp is None else self.jvm.doubles(sumExp))

    def getVectorsMix(self, mixLen):
        mix = None if mixLen is None else self.jvm.doubles(mixLen)
        lam = self.call("nGetVectorsMix", mix)
        return lam, (None if mix is None else mix.get())

    def topWords(self, m, n, K):
        t, c, z = self.jvm.ints(K * n), self.jvm.ints(K * n), self.jvm.ints(K)
        self.call("nTopWords", m, n, t, c, z)
        return t.get().reshape(K, n), c.get().reshape(K, n), z.get()

    def discrWeights(self, numModalities, m, typeWeightLen=None):
        w = self.jvm.doubles(numModalities)
        tw = None if typeWeightLen is None else self.jvm.doubles(typeWeightLen)
        self.call("nDiscrWeights", w, m, tw)
        return w.get(), (None if tw is None else tw.get())

    def diagnostics(self, numTopics, numTypes0, numModalities, numTopWords, wordLength):
        d = JniDiagnostics(self.jvm, numTopics, numTopWords, numTypes0, numModalities)
        self.call("nDiagnostics", numTopWords, None if wordLength is None else self.jvm.ints(wordLength), *d.arrays())
        return d

    def getTuning(self):
        iv, dv = self.jvm.ints(8), self.jvm.doubles(17)
        self.call("nGetTuning", iv, dv)
        iv, dv = iv.get(), dv.get()
        t = Tuning()
        t.forcePrimary, t.narrow, t.walkFixed, t.singleStream, t.live16 = (int(x) for x in iv[:5])
        t.learntWalkStep = [int(iv[5]), int(iv[6]), int(iv[7])]
        t.primaryMinShare = float(dv[0])
        t.walkTheta, t.treeBranchShare = list(dv[1:9]), list(dv[9:17])
        return t

    def setTuning(self, t):
        iv = [t.forcePrimary, t.narrow, t.walkFixed, t.singleStream, t.live16, t.learntWalkStep[0], t.learntWalkStep[1], t.learntWalkStep[2]]
        dv = [t.primaryMinShare] + list(t.walkTheta) + list(t.treeBranchShare)
        self.call("nSetTuning", self.jvm.ints(iv), self.jvm.doubles(dv))

    def close(self):
        if self.handle:
            h, self.handle = self.handle, 0
            self.jvm.call("nDestroy", h)


class JniGroup:                                               # NativeSampler.Group
    def __init__(self, jvm, samplers=None, _g=None):
        self.jvm = jvm
        if _g is not None:
            self.g, self.members = _g, 1
        else:
            hs = [s.handle for s in samplers]
            self.g = 0
            self.g = jvm.call("nGroupCreate", jvm.longs(hs))
            self.members = len(hs)

    @staticmethod
    def ofRank(jvm, sampler, id_, rank, nranks):
        return JniGroup(jvm, _g=jvm.call("nGroupCreateRank", sampler.handle, jvm.bytes(id_), rank, nranks))

    @staticmethod
    def uniqueId(jvm):
        id_ = jvm.bytes(128)
        jvm.call("nGroupUniqueId", id_)
        return id_.get()

    def buildCounts(self):
        self.jvm.call("nGroupBuildCounts", self.g)

    def sweep(self, sweepIdx, seed, flags):
        flat, act = self.jvm.longs(self.members * 8), self.jvm.ints(3)
        exchangeMs = self.jvm.call("nGroupSweep", self.g, sweepIdx, seed, flags, flat, act)
        f, a = flat.get(), act.get()
        out = []
        for i in range(self.members):
            st = _stats_from_flat(f, i)
            st.activatedTopic, st.activatedModality, st.activations, st.totalMs = int(a[0]), int(a[1]), int(a[2]), exchangeMs
            out.append(st)
        return out

    def drain(self):
        self.jvm.call("nGroupDrain", self.g)

    def abort(self):
        self.jvm.call("nGroupAbort", self.g)

    def modelLogLikelihood(self, numModalities):
        ll = self.jvm.doubles(numModalities)
        self.jvm.call("nGroupModelLogLikelihood", self.g, ll)
        return ll.get()

    def getDocTopicHist(self, m, K, histLen, lensLen=0):
        hist, lens = self.jvm.ints(K * histLen), (self.jvm.ints(lensLen) if lensLen else None)
        self.jvm.call("nGroupGetDocTopicHist", self.g, m, hist, histLen, lens)
        return hist.get().reshape(K, histLen), (lens.get() if lens else None)

    def getCountHistogram(self, m, length):
        h = self.jvm.ints(length)
        self.jvm.call("nGroupGetCountHistogram", self.g, m, h)
        return h.get()

    def viewOverlapSums(self, numModalities):
        s = self.jvm.doubles(numModalities * numModalities)
        self.jvm.call("nGroupViewOverlapSums", self.g, s)
        return s.get()

    def gammaDocStatistics(self, m, gammaM, seed, round_):
        o = self.jvm.doubles(2)
        self.jvm.call("nGroupGammaDocStatistics", self.g, m, gammaM, seed, round_, o)
        return o.get()

    def diagnostics(self, numTopics, numTypes0, numModalities, numTopWords, wordLength):
        d = JniDiagnostics(self.jvm, numTopics, numTopWords, numTypes0, numModalities)
        self.jvm.call("nGroupDiagnostics", self.g, numTopWords, None if wordLength is None else self.jvm.ints(wordLength), *d.arrays())
        return d

    def close(self):
        if self.g:
            g, self.g = self.g, 0
            self.jvm.call("nGroupDestroy", g)
