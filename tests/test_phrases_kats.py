"""Known answers for the topic phrases, no GPU: the restatement of findTopicPhrases (tests/phrases_numpy.py) against hand-derived cases,
the order and the cut, merge_topic_phrases over document shards, the new ABI symbol, and the phrases JNI shim by inspection (no JDK here:
type-checked against tests/native/jni_stub, its entry against the native of NativePhrases.java, compiled with the two other shim sources
as one translation unit)."""
import os
import re
import subprocess

import numpy as np
import pytest

from mvtopicmodel_amd import _lib
from mvtopicmodel_amd import native
from tests import jni_harness as H
from tests import phrases_numpy as pn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JAVA_DIR = os.path.join(ROOT, "mvtopicmodel_amd", "java")
SHIM = os.path.join(JAVA_DIR, "mvhdp_phrases_jni.cpp")
JAVA = os.path.join(JAVA_DIR, "org", "madgik", "MVTopicModel", "NativePhrases.java")


def letters(*docs, words=None):
    """documents as strings of topic letters; word ids are the positions within the document unless given: {topic letter: {ids: count}}"""
    topics = sorted(set("".join(docs)))
    z, tok, off = [], [], [0]
    for i, d in enumerate(docs):
        z += [topics.index(c) for c in d]
        tok += list(range(len(d))) if words is None else list(words[i])
        off.append(len(z))
    ph = pn.find_topic_phrases(max(len(topics), 1), off, tok, z)
    return {topics[k]: p for k, p in enumerate(ph) if p}


def test_hand_derived_walks():
    assert letters("AABBC") == {"A": {(0, 1): 1}}                            # B B lost its first token to the break: one phrase
    assert letters("AABBBC") == {"A": {(0, 1): 1}, "B": {(3, 4): 1}}         # the second without w2
    assert letters("AAA") == {}                                              # dropped at the end
    assert letters("AAB") == {"A": {(0, 1): 1}}
    assert letters("AABBCCD") == {"A": {(0, 1): 1}, "C": {(4, 5): 1}}
    assert letters("A") == {} and letters("") == {} and letters("", "A", "") == {}
    assert letters("AAAAB") == {"A": {(0, 1, 2, 3): 1}}
    assert letters("ABAB") == {} and letters("ABBA") == {"B": {(1, 2): 1}}
    assert letters("AABAAB") == {"A": {(0, 1): 1, (3, 4): 1}}                # B is swallowed; the next A starts afresh
    # a phrase never crosses an entity, and nothing carries over
    assert letters("AA", "AB") == {} and letters("AAB", "AAB") == {"A": {(0, 1): 2}}


def test_the_swallowed_token_and_the_length_two_chain():
    # A A B A A B: the first B breaks (A: 0 1) and is swallowed -> EMPTY; A(3) is held, A(4) opens, B(5) breaks: (A: 3 4)
    assert letters("AABAAB", words=[[7, 8, 9, 7, 8, 9]]) == {"A": {(7, 8): 2}}
    # a chain of length-2 runs alternates: every second run loses its first token and so yields nothing
    assert letters("AABBCCDDEEF") == {"A": {(0, 1): 1}, "C": {(4, 5): 1}, "E": {(8, 9): 1}}
    assert letters("XAABBCCDDEEF") == {"A": {(1, 2): 1}, "C": {(5, 6): 1}, "E": {(9, 10): 1}}
    assert letters("XXAABBCCDDEF") == {"X": {(0, 1): 1}, "B": {(4, 5): 1}, "D": {(8, 9): 1}}


def test_keys_are_topic_and_word_sequence():
    # the same word sequence under two topics counts separately
    got = letters("AAB", "BBA", "AAB", words=[[5, 6, 0], [5, 6, 0], [5, 6, 1]])
    assert got == {"A": {(5, 6): 2}, "B": {(5, 6): 1}}
    # a b and a b c are distinct keys
    got = letters("AAB", "AAAB", "AAB", words=[[1, 2, 0], [1, 2, 3, 0], [1, 2, 9]])
    assert got == {"A": {(1, 2): 2, (1, 2, 3): 1}}


TABLE = [{(3, 1): 2, (1, 2): 2, (1, 2, 0): 2, (1,): 2, (9, 9): 5, (0, 7): 1, (0, 6, 1): 1}, {}, {(4, 4): 1}]


def test_tie_order_and_cut_on_a_hand_made_table():
    full = [(9, 9), (1,), (1, 2), (1, 2, 0), (3, 1), (0, 6, 1), (0, 7)]     # count descending; ties ascending, a proper prefix first
    assert [ids for ids, _ in pn.order_and_cut(TABLE[0], -1)] == full
    assert [c for _, c in pn.order_and_cut(TABLE[0], -1)] == [5, 2, 2, 2, 2, 1, 1]
    for n in (0, 1, 3, 5, 7, 20):
        assert [ids for ids, _ in pn.order_and_cut(TABLE[0], n)] == full[:n]
    toff, woff, words, counts, distinct, occ = pn.arrays(TABLE, 3)
    assert list(toff) == [0, 3, 3, 4] and list(counts) == [5, 2, 2, 1]
    assert list(woff) == [0, 2, 3, 5, 7] and list(words) == [9, 9, 1, 1, 2, 4, 4]
    assert list(distinct) == [7, 0, 1] and list(occ) == [15, 0, 1]           # before the cut
    # the binding's order is the restatement's
    assert native._phrase_order(list(TABLE[0].items()), 3) == pn.order_and_cut(TABLE[0], 3)


def random_corpus(D, K, V, seed, max_len=12):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, D)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return off, rng.integers(0, V, off[-1]).astype(np.int32), rng.integers(0, K, off[-1]).astype(np.int32)


def as_result(ph):
    _, _, _, _, distinct, occ = pn.arrays(ph, -1)
    return native.TopicPhrases(pn.lists(ph, -1), distinct, occ, native.PhraseStats())


@pytest.mark.parametrize("nshards", [2, 3])
def test_merge_of_contiguous_shards_is_the_whole_corpus(nshards):
    K, V, D = 3, 4, 400
    off, tok, z = random_corpus(D, K, V, 5)
    whole = pn.find_topic_phrases(K, off, tok, z)
    assert sum(len(p) for p in whole) > 50 and max(max(p.values()) for p in whole) >= 3
    cuts = [D * i // nshards for i in range(nshards + 1)]
    shards = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        shards.append(pn.find_topic_phrases(K, off[a:b + 1] - off[a], tok[off[a]:off[b]], z[off[a]:off[b]]))
    for n in (-1, 0, 1, 20):
        got = native.merge_topic_phrases([as_result(s) for s in shards], n)
        assert got.phrases == pn.lists(whole, n)
        assert pn.merge(shards, n)[1] == pn.lists(whole, n)                  # the reference merge says the same
        assert list(got.distinct) == [len(p) for p in whole] and list(got.occurrences) == [sum(p.values()) for p in whole]
        assert got.stats.kept == sum(len(r) for r in got.phrases)
    cut = as_result(shards[0])
    cut.phrases = [r[:1] for r in cut.phrases]
    with pytest.raises(ValueError):
        native.merge_topic_phrases([cut, as_result(shards[1])], 20)          # a cut shard result cannot be merged exactly


def test_abi_symbol_declared_listed_exported():
    header = open(os.path.join(ROOT, "include", "mvhdp.h")).read()
    assert re.search(r"\bint mvhdp_topic_phrases\(mvhdp_handle h, const mvhdp_phrase_args\* a, int64_t cap_phrases, int64_t cap_words,", header)
    assert "mvhdp_phrase_stats" in header and "hash_bits" in header
    assert "mvhdp_topic_phrases" in _lib.ABI_SYMBOLS
    L = _lib.load_library()
    assert L.mvhdp_topic_phrases.restype is not None
    # without a handle the call is refused, not run
    assert L.mvhdp_topic_phrases(None, None, 0, 0, None, None, None, None, None, None, None, None, None) == -1
    assert [f for f, _ in _lib.PhraseStatsC._fields_] == re.search(r"typedef struct \{ int64_t ([^;]*); \} mvhdp_phrase_stats;", re.sub(r"/\*.*?\*/", "", header)).group(1).replace(" ", "").split(",")


# ---- the JNI shim of NativePhrases, by inspection -----------------------------------------------------------------------------------
def test_phrases_shim_type_checks_and_matches_the_java_class(tmp_path):
    stub = os.path.join(ROOT, "tests", "native", "jni_stub")
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", stub, "-I", inc, SHIM])
    # the shim sources compile together (one translation unit) and apart, and none holds a using-directive
    assert H.check_sources_compile_together_and_apart()
    code = re.sub(r"//[^\n]*", "", open(SHIM).read())
    assert "Critical" not in code                                            # no critical region: the call blocks
    cxx = {"jlong": "long", "jint": "int", "void": "void", "jintArray": "int[]", "jlongArray": "long[]"}
    ent = {name: (cxx[ret], [cxx[p.strip().split()[0]] for p in params.split(",")[2:]])
           for ret, name, params in re.findall(r"JNIEXPORT (\w+) JNICALL Java_org_madgik_MVTopicModel_NativePhrases_(n\w+)\(([^)]*)\)\s*\{", code)}
    nat = {n: (r, [p.split()[0] for p in params.split(",")])
           for r, n, params in re.findall(r"private static native ([\w\[\]]+) (n\w+)\(([^)]*)\);", open(JAVA).read())}
    assert set(ent) == {"nTopicPhrases"} and ent == nat
    called = set(re.findall(r"\b(mvhdp_[a-z_]+)\s*\(", code))
    assert called == {"mvhdp_topic_phrases"}
    assert 'throw_rt(env, s->h, rc, "mvhdp_topic_phrases")' in code          # ... whose message throw_rt (mvhdp_jni_common.h) fetches
    assert len(re.findall(r"\bmvhdp_last_error\(h\)", H.common_header_code())) == 1
    # every array parameter is length-checked before the library call
    for m in re.finditer(r"NativePhrases_(n\w+)\(([^)]*)\)\s*\{", code):
        body = code[m.end():code.index("\n}\n", m.end())]
        before = body[:re.search(r"= mvhdp_\w+\(", body).start()]
        arrays = re.findall(r"j(?:int|long)Array (\w+)", m.group(2))
        assert len(arrays) == 8
        for a in arrays:
            assert re.search(r"(bad_len\(env, %s\b|GetArrayLength\(%s\))" % (a, a), before), (m.group(1), a)
        assert before.count("ExceptionCheck") == 0                          # (the RAII wrappers do it: one ExceptionCheck in front of every Get)
    # the wrappers are the shared header's, and the only way this source takes an array's elements
    common = H.common_header_code()
    assert len(re.findall(r"!e->ExceptionCheck\(\) \? e->Get\w+ArrayElements", common)) == 3 == len(re.findall(r"Get\w+ArrayElements", common))
    assert "ArrayElements" not in code
    # the handle goes through the registry: pinned for the call, never cast
    assert len(re.findall(r"ShardPin pin_\(env, handle\); Shard\* s = pin_\.s;\n    if \(!s\) return", code)) == 1 and "reinterpret_cast" not in code
