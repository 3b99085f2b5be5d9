"""Known answers for the left-to-right held-out estimator, no GPU: the sequential restatement of the contract in include/mvhdp.h
(tests/native/ltr_ref.c through tests/ltr_ref.py) against closed forms and an exact enumeration, the new ABI symbol, and the JNI shim of
NativeHeldout by inspection (no JDK here: type-checked against tests/native/jni_stub, its entry against the native of NativeHeldout.java,
compiled with the three other shim sources as one translation unit)."""
import os
import re
import subprocess

import numpy as np
import pytest

from mvtopicmodel_amd import _lib
from tests import jni_harness as H
from tests import ltr_cases as lc
from tests import ltr_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JAVA_DIR = os.path.join(ROOT, "mvtopicmodel_amd", "java")
SHIM = os.path.join(JAVA_DIR, "mvhdp_heldout_jni.cpp")
JAVA = os.path.join(JAVA_DIR, "org", "madgik", "MVTopicModel", "NativeHeldout.java")


def model(K, V, seed, alpha=0.1):
    rng = np.random.default_rng(seed)
    nwk = rng.integers(0, 40, (V, K)).astype(np.int32)
    nk = (nwk.sum(0) + rng.integers(0, 9, K)).astype(np.int32)             # other shards' tokens: n_k is not the column sum
    a = rng.uniform(0.5 * alpha, 1.5 * alpha, K)
    return nwk, nk, 0.01, a, 1.7 * a.sum()                                   # alphaSum' is a number of its own (gamma * alphaSum), not sum(alpha_k)


@pytest.mark.parametrize("K", [1, 3, 64, 100, 130, 1000])
def test_one_token_document_is_the_prior_predictive_for_any_seed(K):
    nwk, nk, beta, alpha, asum = model(K, 7, K)
    off, tok = np.array([0, 1], dtype=np.int64), np.array([4], dtype=np.int32)
    phi = (nwk[4] + beta) * (1.0 / (nk + beta * 7))
    want = lc.lane_order_total(alpha * phi) / asum                           # sum_k alpha_k phi_w[k] in the header's order, over alphaSum'
    assert abs(want - float((alpha * phi).sum() / asum)) <= (K + 2) * 2.0 ** -53 * want   # (the order moves the last bits only)
    for R in (1, 4):                                                         # R a power of two: S[0] / R is exact
        got = [lr.evaluate(nwk, nk, beta, alpha, asum, off, tok, particles=R, seed=s, resample=rs) for s in (0, 1, 2 ** 40 + 5) for rs in (True, False)]
        for g in got:
            assert g.S[0] / R == want                                        # an equality, for any seed: no draw comes before the first probability
            assert (g.tokens, g.oov, g.visits) == (1, 0, R) and list(g.doc_tokens) == [1]


def test_one_topic_is_a_closed_form_with_out_of_vocabulary_tokens_anywhere():
    V = 5
    nwk, nk, beta, alpha, asum = model(1, V, 3)
    docs = [[1, 2, 3, 0], [V, 1, 2], [1, V + 3, 2, 2], [3, 4, V], [V, V, 2 ** 31 - 1], [], [V, 0, V, 0, V]]
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    tok = np.array([t for d in docs for t in d], dtype=np.int32)
    rinv = 1.0 / (nk[0] + beta * V)
    want = np.zeros(len(tok))
    for d, doc in enumerate(docs):
        seen = 0
        for i, w in enumerate(doc):
            if w < V:
                want[off[d] + i] = ((alpha[0] + float(seen)) * ((nwk[w, 0] + beta) * rinv)) / (asum + float(seen))
                seen += 1
    for seed in (0, 9):
        for rs in (True, False):
            one = lr.evaluate(nwk, nk, beta, alpha, asum, off, tok, particles=1, seed=seed, resample=rs)
            two = lr.evaluate(nwk, nk, beta, alpha, asum, off, tok, particles=2, seed=seed, resample=rs)
            assert np.array_equal(one.S, want) and np.array_equal(two.S, want + want)
            assert list(one.doc_tokens) == [4, 2, 3, 2, 0, 0, 2] and (one.tokens, one.oov) == (13, 9)
            assert one.doc_ll[4] == 0.0 and one.doc_ll[5] == 0.0             # all out of vocabulary, and empty
            # visits: per limit the in-vocabulary positions before it (resample), plus the limit itself when it is in vocabulary
            assert one.visits == (sum(sum(1 for w in doc[:i] if w < V) for doc in docs for i in range(len(doc))) if rs else 0) + 13
            assert two.visits == 2 * one.visits
            assert np.allclose(one.doc_ll, two.doc_ll, rtol=0, atol=1e-12)   # log(2 p) - log 2


def test_position_one_is_unbiased_and_remembers_the_earlier_token():
    exact, a, b, half, forgets = lc.peaked_expectation()
    assert a < exact < b
    for f in forgets:                                                        # a version that forgets w_0 is outside the bound: the test can tell
        assert abs(f - exact) > half
    off, tok = lc.PEAKED_DOC
    for rs in (True, False):
        r = lr.evaluate(lc.PEAKED_NWK, lc.PEAKED_NK, lc.PEAKED_BETA, lc.PEAKED_ALPHA, lc.PEAKED_ALPHA_SUM, off, tok, particles=lc.PEAKED_R, seed=11, resample=rs, want_P=True)
        assert abs(r.S[1] / lc.PEAKED_R - exact) <= half, (r.S[1] / lc.PEAKED_R, exact, half)
        phi0 = (lc.PEAKED_NWK[0] + lc.PEAKED_BETA) / (lc.PEAKED_NK + lc.PEAKED_BETA * 2)
        assert abs(r.S[0] / lc.PEAKED_R - (lc.PEAKED_ALPHA * phi0).sum() / lc.PEAKED_ALPHA_SUM) <= lc.PEAKED_R * 2.0 ** -52   # position 0 has nothing to remember (R additions)
        assert r.P[:, 1].min() >= a * (1 - 1e-12) and r.P[:, 1].max() <= b * (1 + 1e-12) and len(np.unique(r.P[:, 1])) == 3
        assert np.array_equal(r.S, np.add.accumulate(r.P, axis=0)[-1])       # r ascending


def test_resample_changes_later_positions_only():
    """Position 0 never depends on resample.  Position 1 has the same distribution either way (the test above) but not the same draw: with
    resample, z_0 is drawn again under the counter (limit 1, position 0).  For this seed both draws pick the same topic, so position 1
    agrees exactly as well; from position 2 on the chains part."""
    off, tok = np.array([0, 6], dtype=np.int64), np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)
    args = (lc.PEAKED_NWK, lc.PEAKED_NK, lc.PEAKED_BETA, lc.PEAKED_ALPHA, lc.PEAKED_ALPHA_SUM, off, tok)
    on = lr.evaluate(*args, particles=1, seed=0, resample=True)
    no = lr.evaluate(*args, particles=1, seed=0, resample=False)
    assert on.S[0] == no.S[0] and on.S[1] == no.S[1]
    assert (on.S[2:] != no.S[2:]).any()
    assert (on.visits, no.visits) == (21, 6)
    for seed in range(8):                                                    # position 0 for every seed
        assert lr.evaluate(*args, particles=3, seed=seed).S[0] == lr.evaluate(*args, particles=3, seed=seed, resample=False).S[0]


def test_a_range_of_documents_with_its_doc_base_is_the_slice():
    nwk, nk, beta, alpha, asum = model(5, 30, 8)
    off, tok = lc.heldout_docs(30, n_docs=12, seed=4, lengths=[0, 1, 2, 5, 9])
    whole = lr.evaluate(nwk, nk, beta, alpha, asum, off, tok, particles=3, seed=21)
    a, b = 4, 9
    part = lr.evaluate(nwk, nk, beta, alpha, asum, off[a:b + 1] - off[a], tok[off[a]:off[b]], particles=3, seed=21, doc_base=a)
    assert np.array_equal(part.S, whole.S[off[a]:off[b]]) and np.array_equal(part.doc_ll, whole.doc_ll[a:b])
    other = lr.evaluate(nwk, nk, beta, alpha, asum, off[a:b + 1] - off[a], tok[off[a]:off[b]], particles=3, seed=21, doc_base=0)
    assert not np.array_equal(other.S, part.S)                               # the document index is part of the stream
    # the high half of a document index reaches the counter as well
    far = lr.evaluate(nwk, nk, beta, alpha, asum, off, tok, particles=3, seed=21, doc_base=2 ** 32)
    assert not np.array_equal(far.S, whole.S)


def test_the_restatements_philox_is_random123s():
    # Random123 known answers for philox4x32_10
    assert lr.philox([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert lr.philox([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert lr.philox([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_abi_symbol_declared_listed_exported():
    header = open(os.path.join(ROOT, "include", "mvhdp.h")).read()
    assert re.search(r"\bint mvhdp_heldout_left_to_right\(mvhdp_handle h, const mvhdp_heldout_args\* a, int64_t num_docs,", header)
    assert "mvhdp_heldout_left_to_right" in _lib.ABI_SYMBOLS
    L = _lib.load_library()
    assert L.mvhdp_heldout_left_to_right.restype is not None
    # without a handle the call is refused, not run
    assert L.mvhdp_heldout_left_to_right(None, None, 0, None, None, None, None, None, None) == -1
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    st = re.search(r"typedef struct \{ double log_likelihood; int64_t ([^;]*); \} mvhdp_heldout_stats;", plain).group(1).replace(" ", "").split(",")
    assert [f for f, _ in _lib.HeldoutStatsC._fields_] == ["log_likelihood"] + st
    ar = re.search(r"typedef struct \{ ([^}]*)\} mvhdp_heldout_args;", plain).group(1)
    names = [n.strip().lstrip("*") for decl in ar.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].replace("double*", "").replace("const", "").split(",")]
    assert [f for f, _ in _lib.HeldoutArgsC._fields_] == names, names
    # the header's summation paragraph names what the restatement and the kernel share
    for word in ("wave_incl_scan_d_dpp", "bits_to_unit", "Philox4x32-10", "SparseLDA", "vectors mix"):
        assert word in header


# ---- the JNI shim of NativeHeldout, by inspection -----------------------------------------------------------------------------------
def test_heldout_shim_type_checks_and_matches_the_java_class(tmp_path):
    stub = os.path.join(ROOT, "tests", "native", "jni_stub")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", stub, "-I", inc, SHIM])
    # the shim sources compile together (one translation unit) and apart, and none holds a using-directive
    assert H.check_sources_compile_together_and_apart()
    code = re.sub(r"//[^\n]*", "", open(SHIM).read())
    assert "Critical" not in code                                            # no critical region: the call blocks
    cxx = {"jlong": "long", "jint": "int", "jdouble": "double", "void": "void", "jintArray": "int[]", "jlongArray": "long[]", "jdoubleArray": "double[]"}
    ent = {name: (cxx[ret], [cxx[p.strip().split()[0]] for p in params.split(",")[2:]])
           for ret, name, params in re.findall(r"JNIEXPORT (\w+) JNICALL Java_org_madgik_MVTopicModel_NativeHeldout_(n\w+)\(([^)]*)\)\s*\{", code)}
    nat = {n: (r, [p.split()[0] for p in params.split(",")])
           for r, n, params in re.findall(r"private static native ([\w\[\]]+) (n\w+)\(([^)]*)\);", open(JAVA).read())}
    assert set(ent) == {"nLeftToRight"} and ent == nat
    called = set(re.findall(r"\b(mvhdp_[a-z_]+)\s*\(", code))
    assert called == {"mvhdp_heldout_left_to_right"}
    assert 'throw_rt(env, s->h, rc, "mvhdp_heldout_left_to_right")' in code  # ... whose message throw_rt (mvhdp_jni_common.h) fetches
    assert len(re.findall(r"\bmvhdp_last_error\(h\)", H.common_header_code())) == 1
    # every array parameter is length-checked before the library call; the token arrays against the last entry of docOff
    for m in re.finditer(r"NativeHeldout_(n\w+)\(([^)]*)\)\s*\{", code):
        body = code[m.end():code.index("\n}\n", m.end())]
        before = body[:re.search(r"= mvhdp_\w+\(", body).start()]
        arrays = re.findall(r"j(?:int|long|double)Array (\w+)", m.group(2))
        assert len(arrays) == 7
        for a in arrays:
            assert re.search(r"(bad_len\(env, %s\b|GetArrayLength\(%s\))" % (a, a), before), (m.group(1), a)
        assert re.search(r"GetLongArrayRegion\(docOff, \(jsize\)D, 1, &N\)", before) and re.search(r"bad_len\(env, tokens, N,", before)
        assert re.search(r"bad_len\(env, positionSum, N,", before)
    # the wrappers are the shared header's, and the only way this source takes an array's elements
    common = H.common_header_code()
    assert len(re.findall(r"!e->ExceptionCheck\(\) \? e->Get\w+ArrayElements", common)) == 3 == len(re.findall(r"Get\w+ArrayElements", common))
    assert "ArrayElements" not in code
    # the handle goes through the registry: pinned for the call, never cast
    assert len(re.findall(r"ShardPin pin_\(env, handle\); Shard\* s = pin_\.s;\n    if \(!s\) return", code)) == 1 and "reinterpret_cast" not in code
