"""Known answers for the post-training features, no GPU: the numpy restatement (tests/sim_numpy.py) against hand-derived values, the
pure host function mvhdp_sim_probe, the derived margin of the fp32 screen against an fp32 emulation of it, and the new JNI shim by
inspection (no JDK here: type-checked against tests/native/jni_stub, its entries against the natives of NativeSimilarity.java)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import doc_topics as dto
from tests import jni_harness as H
from tests import sim_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "mvtopicmodel_amd", "java", "mvhdp_sim_jni.cpp")
JAVA = os.path.join(ROOT, "mvtopicmodel_amd", "java", "org", "madgik", "MVTopicModel", "NativeSimilarity.java")


def _pairs(x, metric, thr, **kw):
    i, j, s = sn.similar_pairs(np.array(x, dtype=np.float64), metric, thr, **kw)
    return {(int(a), int(b)): float(v) for a, b, v in zip(i, j, s)}


def test_cosine_known_answers():
    # [1,0].[3,4] = 3, |[3,4]| = 5: exactly 0.6
    assert _pairs([[1, 0], [3, 4]], sn.COS, 0.0) == {(0, 1): 0.6}
    assert _pairs([[1, 0], [3, 4]], sn.COS_FOLDED, 0.0) == {(0, 1): 1.0 - abs(1.0 - 0.6)}
    assert _pairs([[1, 0], [3, 4]], sn.COS, 0.6) == {}                       # strict
    assert _pairs([[1, 0], [3, 4]], sn.COS, np.nextafter(0.6, 0)) == {(0, 1): 0.6}
    # identical rows: the cosine may round above 1, the fold brings it back to <= 1
    rng = np.random.default_rng(1)
    for _ in range(50):
        r = rng.random(7)
        got = _pairs([r, r], sn.COS_FOLDED, 0.0)
        assert list(got) == [(0, 1)] and 1.0 - 1e-15 <= got[(0, 1)] <= 1.0
    assert _pairs([[1, 0, 0], [0, 2, 0]], sn.COS, 0.0) == {}                 # orthogonal: 0 is not > 0
    assert _pairs([[1, 1], [0, 0], [1, 1]], sn.COS, 0.0) == {(0, 2): _pairs([[1, 1], [1, 1]], sn.COS, 0.0)[(0, 1)]}   # a zero row never pairs
    # a negative cosine passes through COS unchanged (no pair at threshold 0); the fold sends it further down
    s, ok = sn.sim_matrix(np.array([[1.0, 0.0], [-3.0, 4.0]]), sn.COS)
    assert s[0, 1] == -0.6 and ok.all()
    s, _ = sn.sim_matrix(np.array([[1.0, 0.0], [-3.0, 4.0]]), sn.COS_FOLDED)
    assert s[0, 1] == 1.0 - abs(1.0 - -0.6)
    # min_weight: entries <= it count as 0 (NormWeight > 0.03)
    assert _pairs([[0.03, 1.0], [1.0, 0.03]], sn.COS, 0.0, min_weight=0.03) == {}
    assert list(_pairs([[0.04, 1.0], [1.0, 0.04]], sn.COS, 0.0, min_weight=0.03)) == [(0, 1)]


def test_jsd_known_answers():
    assert _pairs([[0.5, 0.5], [0.5, 0.5]], sn.JSD, 0.0) == {}               # equal rows: every log is log(1) = 0
    s, _ = sn.sim_matrix(np.array([[0.25, 0.75, 0.0], [0.25, 0.75, 0.0]]), sn.JSD)
    assert s[0, 1] == 0.0
    # disjoint rows: every term is p * log(p / (p/2)) = p * log 2, so each KL is log 2 / log 2 = 1 for rows that sum to 1
    s, _ = sn.sim_matrix(np.array([[1.0, 0.0], [0.0, 1.0]]), sn.JSD)
    assert s[0, 1] == 1.0
    s, _ = sn.sim_matrix(np.array([[0.5, 0.5, 0, 0], [0, 0, 0.25, 0.75]]), sn.JSD)
    assert abs(s[0, 1] - 1.0) <= 4 * 2.0 ** -52
    # m_k = 0 under a non-zero p_k (p_k = -q_k): klDivergence returns +inf
    s, _ = sn.sim_matrix(np.array([[1.0, 0.5], [-1.0, 0.5]]), sn.JSD)
    assert s[0, 1] == np.inf


def _tiny_model():
    """One view, K = 5, three entities; entity 0 holds topics 1 and 3 twice each (two equal weights), entity 2 is all topic 4."""
    K = 5
    z = [np.array([1, 3, 3, 1, 0, 2, 2, 2, 4, 4, 4, 4], dtype=np.int32)]
    off = [np.array([0, 5, 8, 12], dtype=np.int64)]
    alpha = np.full((1, K + 1), 0.1)
    prop = dto.doc_topic_proportions(K, off, z, alpha, [0.5], [1.0], [1.0])
    return K, prop


def test_doc_topics_top_order_and_cut():
    K, prop = _tiny_model()
    assert prop[0, 1] == prop[0, 3] > prop[0, 0] > prop[0, 2] == prop[0, 4]
    off, topics, weights = sn.doc_topics_top(prop, 0.0, -1)
    assert list(off) == [0, 5, 10, 15]
    assert list(topics[:5]) == [3, 1, 0, 4, 2]                               # equal weights: the LARGER topic id first (IDSorter.compareTo)
    assert list(topics[5:10]) == [2, 4, 3, 1, 0] and list(topics[10:]) == [4, 3, 2, 1, 0]
    assert np.array_equal(weights, prop[np.repeat(np.arange(3), 5), topics])
    # the oracle's printDocumentTopics walks the same order (its last line per document lists every kept topic)
    text = dto.print_document_topics(prop, ["a", "b", "c"], 0.0, -1, repr).split("\n")
    assert [int(t) for t in text[5].split("\t")[2::2] if t] == [3, 1, 0, 4, 2]
    # cut at the first weight < threshold, and at max
    thr = float(prop[0, 0])
    off, topics, weights = sn.doc_topics_top(prop, thr, -1)
    assert list(topics[off[0]:off[1]]) == [3, 1, 0] and (weights >= thr).all()
    off, topics, _ = sn.doc_topics_top(prop, thr, 1)
    assert list(off) == [0, 1, 2, 3] and list(topics) == [3, 2, 4]
    off, topics, _ = sn.doc_topics_top(prop, 2.0, -1)
    assert list(off) == [0, 0, 0, 0] and len(topics) == 0
    assert list(sn.doc_topics_top(prop, 0.0, K + 7)[0]) == [0, 5, 10, 15]   # max > K: K


def test_distribution_rounding_rule():
    # floor(w * 10^4 + 0.5) / 10^4: half goes up
    assert sn.round_half_up(0.12345, 4) == 0.1235 and sn.round_half_up(0.12344999, 4) == 0.1234
    assert sn.round_half_up(0.00004, 4) == 0.0 and sn.round_half_up(0.00005, 4) == 0.0001
    assert sn.round_half_up(2 / 3, 5) == 0.66667 and sn.round_half_up(0.25, 0) == 0.0 and sn.round_half_up(0.5, 0) == 1.0
    K, prop = _tiny_model()
    thr = float(prop[0, 0])
    out = sn.entity_topic_distributions(prop, thr, -1, -1, [[0], [0, 2], [], [2, 0]])
    r = lambda v: float(sn.round_half_up(v, 4))
    t0 = (r(prop[0, 0]) + r(prop[0, 1])) + r(prop[0, 3])                     # one chain, ascending topic
    assert out[0, 1] == r(prop[0, 1]) / t0 and out[0, 2] == 0.0 and out[0, 4] == 0.0
    assert not out[2].any()                                                  # the empty group
    t1 = t0 + r(prop[2, 4])
    assert out[1, 4] == r(prop[2, 4]) / t1 and out[1, 3] == r(prop[0, 3]) / t1
    t3 = ((r(prop[2, 4]) + r(prop[0, 0])) + r(prop[0, 1])) + r(prop[0, 3])   # member order is part of the definition
    assert out[3, 4] == r(prop[2, 4]) / t3
    out5 = sn.entity_topic_distributions(prop, thr, -1, 5, [[0, 2]])
    assert np.array_equal(out5[0], sn.round_half_up(out[1], 5))
    assert not sn.entity_topic_distributions(prop, 2.0, -1, 5, [[0, 1, 2]]).any()   # total 0: a row of zeros


def test_sim_probe_margins_and_stripes():
    from mvtopicmodel_amd import _lib
    from mvtopicmodel_amd.native import sim_probe, MvhdpError
    L = _lib.load_library()
    for dim in (1, 2, 3, 400, 4096, 65536):
        st = sim_probe(1000, dim)
        assert st.margin == (dim + 4) * 2.0 ** -23 == sn.margin(dim)
    assert sim_probe(10, 65536).margin < 0.01
    st = _lib.SimStatsC()
    assert L.mvhdp_sim_probe(10, 65537, 0, C.byref(st)) == -6               # MVHDP_ERR_UNSUPPORTED
    assert L.mvhdp_sim_probe(10, 0, 0, C.byref(st)) == -1 and L.mvhdp_sim_probe(-1, 4, 0, C.byref(st)) == -1
    assert L.mvhdp_sim_probe(10, 4, -1, C.byref(st)) == -1 and L.mvhdp_sim_probe(10, 4, 0, None) == -1
    with pytest.raises(MvhdpError):
        sim_probe(10, 1 << 20)
    # stripes of S rows; per stripe the 128 x 128 tiles (a, b), b >= a, counted from the stripe's first row
    def cells(n, S):
        tot = 0
        for r0 in range(0, n, S):
            r1 = min(r0 + S, n)
            na, nb = -(-(r1 - r0) // 128), -(-(n - r0) // 128)
            tot += sum(nb - a for a in range(na)) * 128 * 128
        return tot
    for n, S, stripes in ((0, 0, 0), (1, 0, 0), (2, 0, 1), (128, 0, 1), (129, 0, 1), (300, 0, 1), (700, 96, 8), (4096, 0, 1), (4097, 0, 2), (100000, 0, 25), (700, 128, 6)):
        st = sim_probe(n, 400, S)
        assert st.stripes == stripes, (n, S)
        assert st.pairs_screened == (cells(n, S or 4096) if n >= 2 else 0), (n, S)
        assert st.candidates == st.emitted == st.regrown == 0
    assert sim_probe(129, 7).pairs_screened == 3 * 128 * 128               # tiles (0,0), (0,1), (1,1)
    assert sim_probe(700, 400, 96).pairs_screened >= 700 * 699 // 2


def _adversarial_pairs():
    rng = np.random.default_rng(20240611)
    out = []
    for dim in (1, 2, 3, 400, 4096):
        for kind in range(8):
            for rep in range(5):
                a, b = rng.random(dim), rng.random(dim)
                if kind == 1:
                    b = a.copy()                                             # equal rows
                elif kind == 2:
                    a = rng.random(dim) * 1e-6; a[rng.integers(dim)] = 1.0; b = rng.random(dim)   # one dominant entry
                elif kind == 3:
                    a = rng.random(dim) * np.where(np.arange(dim) % 2, -1.0, 1.0); b = np.ones(dim)   # alternating signs: cancellation
                elif kind == 4:
                    a = rng.standard_normal(dim); b = rng.standard_normal(dim)   # signed dense rows, like topic vectors
                elif kind == 5:
                    a = np.where(rng.random(dim) < 0.05, rng.uniform(0.03, 0.6, dim), 0.0); a[0] = 0.3
                    b = np.where(rng.random(dim) < 0.05, rng.uniform(0.03, 0.6, dim), 0.0); b[0] = 0.1   # sparse rows, like entity vectors
                elif kind == 6:
                    a = rng.random(dim) * 1e150; b = rng.random(dim) * 1e-150 + 1e-160   # far apart in magnitude, both inside the screened range
                elif kind == 7:
                    a = np.ones(dim); b = -np.ones(dim)
                out.append((dim, kind, a, b))
    return out


def test_f32_screen_stays_within_half_the_margin():
    """margin(dim) = (dim + 4) * 2^-23 is the error bound taken twice: an emulation of the screen (rows normalised in fp64, stored as
    fp32, one fp32 fma chain) differs from the exact fp64 value by at most half of it."""
    cases = _adversarial_pairs()
    assert len(cases) == 200
    worst = 0.0
    for dim, kind, a, b in cases:
        exact = sn.cosine_matrix(np.array([a, b]), sn.COS)[0][0, 1]
        diff = abs(sn.screen_f32(a, b) - exact)
        worst = max(worst, diff / sn.margin(dim))
        assert diff <= sn.margin(dim) / 2, (dim, kind, diff, sn.margin(dim))
    print(f"largest |screen - exact| / margin over {len(cases)} pairs: {worst:.4f}")


# ---- the JNI shim of NativeSimilarity, by inspection --------------------------------------------------------------------------------
def _shim_entries():
    src = re.sub(r"//[^\n]*", "", open(SHIM).read())
    return {name: (ret, [p.strip().split()[0] for p in params.split(",")][2:])
            for ret, name, params in re.findall(r"JNIEXPORT (\w+) JNICALL Java_org_madgik_MVTopicModel_NativeSimilarity_(n\w+)\(([^)]*)\)\s*\{", src)}


def test_sim_shim_type_checks_and_matches_the_java_class(tmp_path):
    stub = os.path.join(ROOT, "tests", "native", "jni_stub")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", stub, "-I", inc, SHIM])
    # the shim sources compile together (one translation unit) and apart, and none holds a using-directive
    assert H.check_sources_compile_together_and_apart()
    src = open(SHIM).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "Critical" not in code                                            # no critical region: every call blocks
    cxx = {"jlong": "long", "jint": "int", "jdouble": "double", "void": "void", "jintArray": "int[]", "jlongArray": "long[]", "jdoubleArray": "double[]"}
    ent = {n: (cxx[r], [cxx[a] for a in args]) for n, (r, args) in _shim_entries().items()}
    nat = {n: (r, [p.split()[0] for p in params.split(",")])
           for r, n, params in re.findall(r"private static native ([\w\[\]]+) (n\w+)\(([^)]*)\);", open(JAVA).read())}
    assert set(ent) == {"nSimilarPairs", "nDocTopicsTop", "nEntityTopicDistributions"} and ent == nat
    # every entry reaches its library function; the shim calls nothing else of the library but mvhdp_last_error
    called = set(re.findall(r"\b(mvhdp_[a-z_]+)\s*\(", code))
    assert called == {"mvhdp_similar_pairs", "mvhdp_doc_topics_top", "mvhdp_entity_topic_distributions"}
    for fn in called:                                                        # ... whose message throw_rt (mvhdp_jni_common.h) fetches
        assert re.search(r'throw_rt\(env, s->h, rc, "%s"\)' % fn, code), fn
    assert len(re.findall(r"\bmvhdp_last_error\(h\)", H.common_header_code())) == 1
    # every array parameter of every entry is length-checked before the library call
    for m in re.finditer(r"NativeSimilarity_(n\w+)\(([^)]*)\)\s*\{", code):
        body = code[m.end():code.index("\n}\n", m.end())]
        before = body[:re.search(r"= mvhdp_\w+\(", body).start()]
        for a in re.findall(r"j(?:int|long|double)Array (\w+)", m.group(2)):
            assert re.search(r"(bad_len\(env, %s\b|GetArrayLength\(%s\))" % (a, a), before), (m.group(1), a)
        assert before.count("ExceptionCheck") == 0                          # (the RAII wrappers do it: one ExceptionCheck in front of every Get)
    # the wrappers are the shared header's, and the only way this source takes an array's elements
    common = H.common_header_code()
    assert len(re.findall(r"!e->ExceptionCheck\(\) \? e->Get\w+ArrayElements", common)) == 3 == len(re.findall(r"Get\w+ArrayElements", common))
    assert "ArrayElements" not in code
    # the handle goes through the registry: pinned for the call, never cast
    assert len(re.findall(r"ShardPin pin_\(env, handle\); Shard\* s = pin_\.s;\n    if \(!s\) return", code)) == 3 and "reinterpret_cast" not in code
