"""mvhdp_topic_gram without a device: the entry through every layer (header, loader, library export, wrappers, build list, documents), and
the sequential restatement of its contract (tests/native/gram_ref.c) against exact rationals on a hand-sized case, its sensitivity to the
order the contract fixes, and the host merge against the restated parts."""
import ctypes as C
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import gram_cases as gc
from tests import gram_ref as gr
from tests.helpers import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mvhdp_topic_gram"
ARGS_FIELDS = ["source", "m", "transform", "blocks_per_pass", "view_weights", "x", "r0", "r1", "threshold"]
STATS_FIELDS = ["rows", "blocks", "passes", "kernel_ms"]


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_entry_exists_in_every_layer():
    hdr = read("include", "mvhdp.h")
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(\s*mvhdp_handle\s+h\s*,\s*const\s+mvhdp_topic_gram_args\s*\*" % NAME, code)
    assert re.search(r"#define\s+MVHDP_GRAM_BLOCK_ROWS\s+1024\b", code)
    assert re.search(r"MVHDP_GRAM_ENTITIES\s*=\s*0\s*,\s*MVHDP_GRAM_WORDS\s*=\s*1\s*,\s*MVHDP_GRAM_HOST\s*=\s*2", code)
    assert re.search(r"MVHDP_GRAM_IDENTITY\s*=\s*0\s*,\s*MVHDP_GRAM_SQRT\s*=\s*1", code)
    for name, fields in (("mvhdp_topic_gram_args", ARGS_FIELDS), ("mvhdp_topic_gram_stats", STATS_FIELDS)):
        st = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, code)
        assert st and [f.split()[-1].lstrip("*") for f in re.split(r"[;,]", st.group(1)) if f.strip()] == fields, name
    for phrase in ("gram_ref.c", "p = fma(y_r[k], y_r[l], p)", "g = g + P_b[k][l]", "q = q + y_r[k]", "its size is part of", "symmetric in every bit",
                   "X_r[k] > threshold", "before the transform", "the comparison is strict", "mvhdp_doc_topic_proportions(h, view_weights, r, r + 1)",
                   "correctly rounded", "(56 bytes)", "(24 bytes)", "No floating-point atomics", "blocks == 0", "It changes no result"):
        assert phrase in hdr, phrase
    from mvtopicmodel_amd import _lib, native
    assert NAME in _lib.ABI_SYMBOLS
    assert [f[0] for f in _lib.TopicGramArgsC._fields_] == ARGS_FIELDS and C.sizeof(_lib.TopicGramArgsC) == 56
    assert [f[0] for f in _lib.TopicGramStatsC._fields_] == STATS_FIELDS and C.sizeof(_lib.TopicGramStatsC) == 24
    L = _lib.load_library()
    assert len(L.mvhdp_topic_gram.argtypes) == 7 and L.mvhdp_topic_gram.restype is C.c_int
    assert L.mvhdp_topic_gram(None, None, None, None, None, None, None) == -1                   # a NULL handle: no device touched
    sig = inspect.signature(native.NativeSampler.topic_gram).parameters
    assert list(sig) == ["self", "source", "m", "view_weights", "r0", "r1", "transform", "threshold", "blocks_per_pass"]
    assert (sig["m"].default, sig["r0"].default, sig["r1"].default, sig["transform"].default, sig["threshold"].default, sig["blocks_per_pass"].default) == \
           (0, 0, None, "identity", None, 0)
    assert list(inspect.signature(native.NativeGroup.topic_gram).parameters)[:2] == ["self", "source"]
    assert [f for f in native.TopicGram.__dataclass_fields__] == ["gram", "sums", "n_above", "co_above", "rows", "transform", "stats"]
    for method in ("cosine", "correlation", "bhattacharyya", "hellinger", "jaccard", "npmi"):
        assert "host derivation" in getattr(native.TopicGram, method).__doc__.lower(), method
    assert "member-order sum" in native.NativeGroup.topic_gram.__doc__ and "integers" in native.NativeGroup.topic_gram.__doc__
    assert callable(native.merge_topic_grams)
    make = read("mvtopicmodel_amd", "csrc", "Makefile")
    assert "mvhdp_gram.hip" in re.search(r"^SRCS\s*=(.*)$", make, flags=re.M).group(1)
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md", "CHANGELOG.md"):
        assert NAME in read(doc), doc
    assert "7i" in read("DESIGN.md") and "CalcTopicSimilarities" in read("INTEGRATION.md") and "topic_gram(" in read("INTEGRATION.md")
    log = read("CHANGELOG.md")
    for not_done in ("a JNI class", "mvhdp_group_", "JSD between topics", "weighted rows", "vectors mix"):
        assert not_done in log, not_done


# ---- the hand-sized case: 7 rows, K = 3, dyadic entries that are perfect squares, so that every product, sum and root is exact ----
X = np.array([[0.25, 4.0, 0.0], [1.0, 0.0, 0.0625], [2.25, 0.25, 9.0], [0.0, 0.0, 1.0], [16.0, 0.5625, 0.25], [0.25, 0.25, 0.25], [0.0, 1.0, 4.0]])


def exact(x, transform):
    y = [[Fraction(v) for v in row] for row in (np.sqrt(x) if transform == "sqrt" else x)]
    K = x.shape[1]
    g = np.array([[float(sum(r[k] * r[l] for r in y)) for l in range(K)] for k in range(K)])
    return g, np.array([float(sum(r[k] for r in y)) for k in range(K)])


def chained(x, transform, B):
    """the contract's order by exact rationals, every step rounded on its own: blocks of B rows"""
    y = np.sqrt(x) if transform == "sqrt" else x
    n, K = y.shape
    g, s = np.zeros((K, K)), np.zeros(K)
    for k in range(K):
        for l in range(K):
            for b0 in range(0, n, B):
                p = 0.0
                for r in range(b0, min(b0 + B, n)):
                    p = float(Fraction(y[r, k]) * Fraction(y[r, l]) + Fraction(p))
                g[k, l] = g[k, l] + p
        for b0 in range(0, n, B):
            q = 0.0
            for r in range(b0, min(b0 + B, n)):
                q = q + y[r, k]
            s[k] = s[k] + q
    return g, s


def test_the_restatement_equals_exact_rationals_on_the_hand_sized_case():
    assert (np.sqrt(X) ** 2 == X).all()
    for transform in ("identity", "sqrt"):
        want = exact(X, transform)
        for variant, block in ((gr.CONTRACT, 1024), (gr.OTHER_BLOCK, 2), (gr.OTHER_BLOCK, 3), (gr.ONE_CHAIN, 1024)):
            got = gr.gram(X, transform, variant, block)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (transform, variant, block)
        assert np.array_equal(bits(want[0]), bits(want[0].T))
    # entries that are not exact: the chain, each fma rounded once, by rationals; blocks of 3 rows through the variant that takes a size
    rng = np.random.default_rng(5)
    x = rng.random((10, 3))
    for transform in ("identity", "sqrt"):
        for B in (3, 4, 1024):
            want = chained(x, transform, B)
            got = gr.gram(x, transform, gr.OTHER_BLOCK, B)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (transform, B)
    assert np.array_equal(bits(gr.gram(x)[0]), bits(gr.gram(x, variant=gr.OTHER_BLOCK, block=1024)[0]))
    # the integers: strict, on X
    na, co = gr.counts(X, 0.25)
    assert na.tolist() == [3, 3, 3] and co.tolist() == [[3, 1, 1], [1, 3, 1], [1, 1, 3]]       # rows {1, 2, 4}, {0, 4, 6}, {2, 3, 6}
    na, co = gr.counts(X, -np.inf)
    assert na.tolist() == [7, 7, 7] and (co == 7).all()
    na, co = gr.counts(X, np.inf)
    assert not na.any() and not co.any()
    g, s = gr.gram(np.zeros((0, 3)))
    assert not bits(g).any() and not bits(s).any()                           # no rows: +0.0 everywhere


def test_every_variant_of_the_order_moves_a_bit():
    """what the device test can tell apart: on about 3000 rows each other order gives another bit pattern somewhere in gram"""
    x = gc.rows(3 * 1024 + 5, 4, seed=1)
    for transform in ("identity", "sqrt"):
        ref = gr.gram(x, transform)
        for variant, block in ((gr.DESCENDING, 1024), (gr.UNFUSED, 1024), (gr.OTHER_BLOCK, 512), (gr.ONE_CHAIN, 1024)):
            other = gr.gram(x, transform, variant, block)
            assert (bits(other[0]) != bits(ref[0])).any(), (transform, variant)
            assert np.allclose(other[0], ref[0], rtol=1e-12, atol=0) and np.allclose(other[1], ref[1], rtol=1e-12, atol=0)
        assert np.array_equal(bits(ref[0]), bits(ref[0].T))
    assert (bits(gr.gram(x, variant=gr.OTHER_BLOCK, block=512)[1]) != bits(gr.gram(x)[1])).any()         # sums follow the blocks as well


def test_merge_of_restated_parts():
    from mvtopicmodel_amd.native import TopicGram, merge_topic_grams
    x = gc.rows(2500, 5, seed=2)
    cuts = [0, 700, 701, 2500]
    for transform in ("identity", "sqrt"):
        parts = [gr.topic_gram(x[a:b], transform, gc.THRESHOLD) for a, b in zip(cuts, cuts[1:])]
        got = merge_topic_grams(parts)
        g = (parts[0].gram + parts[1].gram) + parts[2].gram
        s = (parts[0].sums + parts[1].sums) + parts[2].sums
        assert np.array_equal(bits(got.gram), bits(g)) and np.array_equal(bits(got.sums), bits(s))
        whole = gr.topic_gram(x, transform, gc.THRESHOLD)
        assert np.array_equal(got.n_above, whole.n_above) and np.array_equal(got.co_above, whole.co_above) and got.n_above.dtype == np.int64
        assert got.rows == 2500 and got.transform == transform and isinstance(got, TopicGram)
        assert np.allclose(got.gram, whole.gram, rtol=1e-12)                  # near a single call's sums, not their bits
        back = merge_topic_grams(parts[::-1])
        assert np.array_equal(back.n_above, got.n_above) and np.array_equal(back.co_above, got.co_above)
    no_counts = merge_topic_grams([gr.topic_gram(x[:100]), gr.topic_gram(x[100:])])
    assert no_counts.n_above is None and no_counts.co_above is None
    with pytest.raises(ValueError):
        merge_topic_grams([gr.topic_gram(x[:10], "sqrt"), gr.topic_gram(x[10:20], "identity")])
    with pytest.raises(ValueError):
        merge_topic_grams([])


def test_the_host_derivations():
    """cosine, correlation, Bhattacharyya / Hellinger, Jaccard and NPMI against their definitions in numpy on the rows themselves"""
    x = gc.rows(900, 6, seed=3)
    x /= x.sum(0)                                                            # columns that are distributions, as phi's are
    t = gr.topic_gram(x, "identity", 1e-3)
    norm = np.sqrt((x * x).sum(0))
    assert np.allclose(t.cosine(), (x.T @ x) / np.outer(norm, norm), rtol=1e-12)
    assert np.allclose(t.correlation(), np.corrcoef(x.T), rtol=1e-9, atol=1e-12)
    above = x > 1e-3
    both = (above[:, :, None] & above[:, None, :]).sum(0)
    either = (above[:, :, None] | above[:, None, :]).sum(0)
    assert np.allclose(t.jaccard(), both / either)
    pk, pkl = above.mean(0), both / len(x)
    assert np.allclose(t.npmi(), np.log(pkl / np.outer(pk, pk)) / -np.log(pkl)) and np.allclose(np.diag(t.npmi()), 1.0)
    q = gr.topic_gram(x, "sqrt")
    bc = np.sqrt(x).T @ np.sqrt(x)
    assert np.allclose(q.bhattacharyya(), bc, rtol=1e-12) and np.allclose(q.hellinger(), np.sqrt(np.clip(1.0 - bc, 0.0, None)), atol=1e-7)
    with pytest.raises(ValueError):
        q.cosine()
    with pytest.raises(ValueError):
        q.jaccard()
    with pytest.raises(ValueError):
        t.bhattacharyya()
