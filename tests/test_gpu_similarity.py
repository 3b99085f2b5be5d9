"""mvhdp_similar_pairs, mvhdp_doc_topics_top and mvhdp_entity_topic_distributions on a device against tests/sim_numpy.py.

The cosine metrics are compared bit for bit (pairs and values, whole sets); the JSD by set and within the bound derived below.  The
fp32 screen is held to its contract -- it never decides: whatever it lets through is recomputed, and what it may let through is bounded
by the derived margin -- through the call's own statistics.  Shapes: one k-step, an odd k tail, the BASELINE topic counts; n at and
around the 32- and 128-wide tile edges; ragged stripes; the regrow path of the candidate buffer."""
import ctypes as C

import numpy as np
import pytest

from mvtopicmodel_amd import MvhdpError, NativeSampler, _lib
from mvtopicmodel_amd.native import round_similarity, sim_probe
from tests import jni_harness as H
from tests import sim_numpy as sn
from tests.helpers import INV, golden_sampler
from tests.native_build import jvm  # noqa: F401

pytestmark = pytest.mark.gpu
DIMS = [1, 2, 3, 33, 100, 400, 1000]
NS = [1, 2, 31, 32, 33, 127, 128, 129, 300]
THRESHOLDS = [0.0, 0.15, 0.3, 0.9]


@pytest.fixture(scope="module")
def s():
    with NativeSampler(4, [8]) as smp:                                      # similar_pairs reads no model state: any handle will do
        yield smp


def entity_rows(n, dim, seed):
    """non-negative sparse rows like entity vectors: most entries 0, a few in (0.03, 0.6]; every row keeps at least one entry"""
    rng = np.random.default_rng(seed)
    x = np.where(rng.random((n, dim)) < min(1.0, 6.0 / dim), rng.uniform(0.031, 0.6, (n, dim)), 0.0)
    x[np.arange(n), rng.integers(0, dim, n)] = rng.uniform(0.031, 0.6, n)
    return x


def topic_rows(n, dim, seed):
    """signed dense rows like topic vectors"""
    return np.random.default_rng(seed).standard_normal((n, dim))


def restated(x, min_weight=-np.inf):
    """{metric: (sim matrix, can_pair)} with one pass over the chain"""
    xc = sn.clean(x, min_weight)
    c, na = sn.cosine_matrix(xc, sn.COS)
    ok = (na > 0) & np.isfinite(na)
    with np.errstate(all="ignore"):
        return {sn.COS: (c, ok), sn.COS_FOLDED: (1.0 - np.abs(1.0 - c), ok)}


def assert_same_pairs(got, want, what):
    i, j, v = got[:3]
    wi, wj, wv = want
    assert len(i) == len(wi), (what, len(i), len(wi))
    assert np.array_equal(i, wi) and np.array_equal(j, wj), what
    assert v.tobytes() == wv.tobytes(), (what, np.flatnonzero(v != wv)[:5])


def check_stats(st, mat, thr, n, dim, stripe_rows, count):
    """the screen does its job without deciding"""
    sim, ok = mat
    assert st.emitted == count and st.candidates >= st.emitted
    with np.errstate(invalid="ignore"):
        may = np.triu(sim > thr - 2 * sn.margin(dim), 1) & ok[:, None] & ok[None, :]
    assert st.candidates <= int(may.sum()), (st, int(may.sum()))
    pr = sim_probe(n, dim, stripe_rows)
    assert (st.pairs_screened, st.stripes, st.margin) == (pr.pairs_screened, pr.stripes, pr.margin)


@pytest.mark.parametrize("dim", DIMS)
def test_cosine_pairs_equal_the_restatement_bit_for_bit(s, dim):
    for n in NS:
        for kind, rows in (("entity", entity_rows), ("topic", topic_rows)):
            x = rows(n, dim, 1000 * dim + n)
            mats = restated(x)
            for metric in (sn.COS_FOLDED, sn.COS):
                for thr in THRESHOLDS:
                    got = s.similar_pairs(x, metric, thr)
                    assert_same_pairs(got, sn.similar_pairs(x, metric, thr, matrix=mats[metric]), (kind, n, dim, metric, thr))
                    check_stats(got[3], mats[metric], thr, n, dim, 0, len(got[0]))
                    assert got[3].regrown == 0


def test_ragged_stripes_and_the_regrow_path(s):
    n, dim = 700, 100
    x = entity_rows(n, dim, 7)
    mats = restated(x)
    for metric in (sn.COS_FOLDED, sn.COS):
        want = sn.similar_pairs(x, metric, 0.15, matrix=mats[metric])
        assert len(want[0]) > 1000                                          # (the case has something to find)
        got = s.similar_pairs(x, metric, 0.15, stripe_rows=96)
        assert_same_pairs(got, want, ("stripes", metric))
        check_stats(got[3], mats[metric], 0.15, n, dim, 96, len(want[0]))
        assert got[3].stripes == 8 and got[3].regrown == 0
        small = s.similar_pairs(x, metric, 0.15, stripe_rows=96, candidate_capacity=8)
        assert_same_pairs(small, want, ("regrown", metric))
        assert small[3].regrown >= 1 and small[3].candidates == got[3].candidates
    dense = topic_rows(300, 33, 5)
    got = s.similar_pairs(dense, sn.COS, 0.0, stripe_rows=1, candidate_capacity=1)   # one row per stripe
    assert_same_pairs(got, sn.similar_pairs(dense, sn.COS, 0.0), "one-row stripes")
    assert got[3].stripes == 300


def test_near_ties_are_decided_by_the_exact_stage(s):
    """threshold = the pair's own restated value: absent (strict >); one ulp below: present.  Pairs in a diagonal tile, in the last ragged
    tile and across a stripe border (stripes of 96 rows: 95 | 96)."""
    n, dim = 300, 33
    x = np.random.default_rng(11).random((n, dim))                          # positive rows: every cosine is a usable threshold
    mats = restated(x)
    for metric in (sn.COS_FOLDED, sn.COS):
        sim = mats[metric][0]
        for (i, j) in ((5, 9), (290, 299), (95, 96), (0, 299), (127, 128)):
            v = float(sim[i, j])
            assert 0.0 < v < 1.0
            for thr, present in ((v, False), (np.nextafter(v, 0.0), True)):
                gi, gj, gv, st = s.similar_pairs(x, metric, thr, stripe_rows=96)
                hit = np.flatnonzero((gi == i) & (gj == j))
                assert (len(hit) == 1) == present, (metric, i, j, thr)
                if present:
                    assert gv[hit[0]] == v
                assert_same_pairs((gi, gj, gv), sn.similar_pairs(x, metric, thr, matrix=mats[metric]), (metric, i, j, present))


def test_degenerate_rows_and_the_argument_contract(s):
    n, dim = 140, 33
    x = entity_rows(n, dim, 3)
    x[3] = 0.0                                                              # an all-zero row
    x[130] = 0.0; x[130, :4] = 0.02                                         # emptied by min_weight
    x[7] = 0.0; x[7, 2:9] = 1e-170                                          # norm^2 underflows to 0
    x[129] = 0.0; x[129, 1:5] = 1e200                                       # norm^2 overflows
    x[64] = np.nan                                                          # norm NaN
    x[9] = x[10] * 1e-160                                                   # not screened (fp64 underflow territory), still exact
    x[131] = x[12] * 1e153                                                  # not screened (entries beyond 2^500), norm still finite
    mw = 0.03
    for mw, dead in ((0.03, [3, 130, 7, 129, 64, 9]), (-np.inf, [3, 7, 129, 64])):   # (the filter empties the tiny row 9 as well)
        mats = restated(x, mw)
        ok = mats[sn.COS][1]
        assert not ok[dead].any() and ok[131] and ok.sum() == n - len(dead)
        for metric in (sn.COS_FOLDED, sn.COS):
            for thr in (0.0, 0.15):
                got = s.similar_pairs(x, metric, thr, min_weight=mw)
                assert_same_pairs(got, sn.similar_pairs(x, metric, thr, min_weight=mw, matrix=mats[metric]), (mw, metric, thr))
                for r in dead:
                    assert not ((got[0] == r) | (got[1] == r)).any()
                assert got[3].emitted == len(got[0]) <= got[3].candidates
    assert ((got[0] == 9) | (got[1] == 9)).any() and ((got[0] == 131) | (got[1] == 131)).any()   # the unscreened rows do pair
    mw = 0.03
    mats = restated(x, mw)
    # the contract of the arguments
    for thr in (np.nan, -0.1, np.inf, -np.inf):
        with pytest.raises(MvhdpError) as e:
            s.similar_pairs(x, sn.COS, thr)
        assert e.value.code == INV
    with pytest.raises(MvhdpError) as e:
        s.similar_pairs(np.zeros((2, 65537)), sn.COS, 0.1)
    assert e.value.code == -6                                               # MVHDP_ERR_UNSUPPORTED
    want = sn.similar_pairs(x, sn.COS, 0.15, min_weight=mw, matrix=mats[sn.COS])
    assert s.similar_pairs(x, sn.COS, 0.15, min_weight=mw, count_only=True)[0] == len(want[0]) > 3
    a = _lib.SimArgsC(sn.COS, n, dim, x.ctypes.data, mw, 0.15, 0, 0)
    cap = 3                                                                 # too small: outputs untouched, count right
    gi, gj, gv = np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7.0)
    cnt, st = C.c_int64(), _lib.SimStatsC()
    rc = s.L.mvhdp_similar_pairs(s.h, C.byref(a), cap, gi.ctypes.data, gj.ctypes.data, gv.ctypes.data, C.byref(cnt), C.byref(st))
    assert rc == INV and cnt.value == len(want[0]) and (gi == -7).all() and (gj == -7).all() and (gv == -7.0).all()
    assert b"cap" in s.L.mvhdp_last_error(s.h)
    cap = len(want[0])                                                      # exactly enough
    gi, gj, gv = np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7.0)
    assert s.L.mvhdp_similar_pairs(s.h, C.byref(a), cap, gi.ctypes.data, gj.ctypes.data, gv.ctypes.data, C.byref(cnt), None) == 0
    assert_same_pairs((gi[:cap], gj[:cap], gv[:cap]), want, "exact cap")
    assert gi[cap] == -7 and gv[cap] == -7.0
    # the flow's rounding lives in the binding
    assert np.array_equal(round_similarity([0.1234, 0.1235, 0.9995]), [0.123, 0.124, 1.0])
    # n < 2: nothing to compare
    assert s.similar_pairs(x[:1], sn.COS, 0.0, count_only=True)[0] == 0 and s.similar_pairs(np.zeros((0, 4)), sn.COS, 0.0, count_only=True)[0] == 0


def prob_rows(n, dim, seed):
    rng = np.random.default_rng(seed)
    x = np.where(rng.random((n, dim)) < min(1.0, 5.0 / dim), rng.random((n, dim)), 0.0)
    x[np.arange(n), rng.integers(0, dim, n)] += rng.random(n) + 0.1
    return x / x.sum(axis=1, keepdims=True)


@pytest.mark.parametrize("n,dim", [(2, 3), (33, 2), (33, 33), (129, 100), (300, 33), (40, 400)])
def test_jsd_pairs_and_values(s, n, dim):
    """Java's Math.log and the device's log may differ by an ulp, so the set is compared on inputs that keep every pair 1e-9 away from
    the threshold (checked here first), and values within 8 * dim * 2^-52 * (sum p + sum q): a few ulp each for the division, the log and
    the product of a term that is at most its p_k, over a chain of dim terms."""
    x = prob_rows(n, dim, 50 + n + dim)
    sim, ok = sn.sim_matrix(x, sn.JSD)
    assert ok.all()
    worst = 0.0
    for thr in (0.15, 0.5, 0.02):
        iu = np.triu_indices(n, 1)
        assert (np.abs(sim[iu] - thr) > 1e-9).all(), "the fixture has a pair within 1e-9 of the threshold: reseed"
        wi, wj, wv = sn.similar_pairs(x, sn.JSD, thr, matrix=(sim, ok))
        gi, gj, gv, st = s.similar_pairs(x, sn.JSD, thr, stripe_rows=96 if n > 200 else 0)
        assert np.array_equal(gi, wi) and np.array_equal(gj, wj), (n, dim, thr)
        bound = 8 * dim * 2.0 ** -52 * (x.sum(axis=1)[wi] + x.sum(axis=1)[wj])
        diff = np.abs(gv - wv)
        worst = max(worst, float(diff.max()) if len(diff) else 0.0)
        assert (diff <= bound).all(), (n, dim, thr, float(diff.max()))
        assert st.emitted == len(gi) and st.margin == 0.0
    print(f"JSD n={n} dim={dim}: largest |device - restatement| = {worst:.3e}")
    # equal rows: 0 is not > 0; disjoint rows: exactly 1
    assert s.similar_pairs(np.array([[0.5, 0.5], [0.5, 0.5]]), sn.JSD, 0.0, count_only=True)[0] == 0
    gi, gj, gv, _ = s.similar_pairs(np.array([[1.0, 0.0], [0.0, 1.0]]), sn.JSD, 0.0)
    assert (list(gi), list(gj), list(gv)) == ([0], [1], [1.0])


# ---- thresholded topic lists and entity distributions -------------------------------------------------------------------------------
W3 = np.array([1.0, 0.7, 0.4])
CUTS = [(0.0, -1), (0.03, -1), (0.03, 3), (0.5, 1)]


def groups_of(D, prop):
    rng = np.random.default_rng(D)
    return [[d] for d in range(D)] + [list(range(D)), list(range(0, D, 2)), list(range(D // 3, D)), [], list(rng.permutation(D)[:9]) + [4, 4]]


@pytest.mark.parametrize("name", ["m3_k20", "m3_k100_inactive"])
def test_topic_lists_and_entity_distributions_on_the_goldens(s, name):
    smp, g, _ = golden_sampler(name)
    with smp:
        D, K = smp.D, smp.K
        assert any((np.diff(g[f"doc_off{m}"]) == 0).any() for m in (1, 2))  # entities without a side view are in
        prop = smp.doc_topic_proportions(W3)
        for thr, mx in CUTS:
            off, topics, weights = smp.doc_topics_top(W3, thr, mx)
            woff, wtopics, wweights = sn.doc_topics_top(prop, thr, mx)
            assert np.array_equal(off, woff) and np.array_equal(topics, wtopics), (thr, mx)
            assert weights.tobytes() == wweights.tobytes()                  # the bits of mvhdp_doc_topic_proportions
            o2, t2, w2 = smp.doc_topics_top(W3, thr, mx, 7, 23)             # a window
            assert np.array_equal(o2, woff[7:24] - woff[7]) and np.array_equal(t2, wtopics[woff[7]:woff[23]]) and w2.tobytes() == wweights[woff[7]:woff[23]].tobytes()
        assert len(smp.doc_topics_top(W3, 0.0, -1)[1]) == D * K and len(smp.doc_topics_top(W3, 0.5, 1, 5, 5)[1]) == 0
        # capacity protocol
        woff, wtopics, _ = sn.doc_topics_top(prop, 0.03, -1)
        w = np.ascontiguousarray(W3)
        cnt = C.c_int64()
        t, wt = np.full(4, -7, np.int32), np.full(4, -7.0)
        rc = smp.L.mvhdp_doc_topics_top(smp.h, w.ctypes.data, 0, D, 0.03, -1, 4, None, t.ctypes.data, wt.ctypes.data, C.byref(cnt))
        assert rc == INV and cnt.value == len(wtopics) > 4 and (t == -7).all() and (wt == -7.0).all()
        assert smp.L.mvhdp_doc_topics_top(smp.h, w.ctypes.data, 0, D, 0.03, -1, 0, None, None, None, C.byref(cnt)) == 0 and cnt.value == len(wtopics)
        # groups: singletons, everyone, overlapping, empty, repeated members; and one whose total is 0
        groups = groups_of(D, prop)
        for thr, mx in CUTS:
            for digits in (5, -1):
                got = smp.entity_topic_distributions(W3, thr, groups, mx, digits)
                want = sn.entity_topic_distributions(prop, thr, mx, digits, groups)
                assert got.tobytes() == want.tobytes(), (thr, mx, digits, np.argwhere(got != want)[:4])
                assert got.tobytes() == smp.entity_topic_distributions(W3, thr, groups, mx, digits).tobytes()   # two calls, the same bits
        none = smp.entity_topic_distributions(W3, 2.0, [[0, 1, 2], []])    # no weight reaches 2: totals 0
        assert none.shape == (2, K) and not none.any()
        with pytest.raises(MvhdpError):
            smp.entity_topic_distributions(W3, 0.03, [[D]])
        # end to end: the distributions into similar_pairs
        dist = smp.entity_topic_distributions(W3, 0.03, groups[:D + 3], -1, 5)
        for metric, thr in ((sn.COS_FOLDED, 0.15), (sn.COS, 0.3)):
            assert_same_pairs(s.similar_pairs(dist, metric, thr, min_weight=0.03), sn.similar_pairs(dist, metric, thr, min_weight=0.03), (name, metric))
            assert len(sn.similar_pairs(dist, metric, thr, min_weight=0.03)[0]) > 0


# ---- the Java path: the four shim sources as one library, under the test-side JNIEnv (tests/jni_harness.py) ---------------------------
IAE = "java/lang/IllegalArgumentException"


def test_the_java_entries_equal_the_binding(jvm):
    smp, g, hy = golden_sampler("m3_k20")
    with smp:
        D, K, M = smp.D, smp.K, smp.M
        j = H.JniSampler(jvm, K, smp.V)
        try:
            for m in range(M):
                j.setCorpus(m, g[f"doc_off{m}"], g[f"tokens{m}"])
                j.setAssignments(m, smp.get_assignments(m))
            j.setHyper(hy.alpha, hy.alpha_sum, hy.beta, hy.beta_sum, hy.gamma, hy.p_a, hy.p_b, hy.inactive)
            j.buildCounts()
            h = j.handle
            # nDocTopicsTop: count first, then the arrays
            off, topics, weights = smp.doc_topics_top(W3, 0.03, 3)
            joff = jvm.longs(D + 1)
            n = jvm.call("nDocTopicsTop", h, jvm.doubles(W3), 0, D, 0.03, 3, joff, None, None)
            assert n == len(topics) and np.array_equal(joff.get(), off)
            jt, jw = jvm.ints(n), jvm.doubles(n)
            assert jvm.call("nDocTopicsTop", h, jvm.doubles(W3), 0, D, 0.03, 3, None, jt, jw) == n
            assert np.array_equal(jt.get(), topics) and jw.get().tobytes() == weights.tobytes()
            jt2, jw2 = jvm.ints([-7] * 2), jvm.doubles([-7.0] * 2)               # too small: the count, arrays untouched, no exception
            assert jvm.call("nDocTopicsTop", h, jvm.doubles(W3), 0, D, 0.03, 3, None, jt2, jw2) == n
            assert (jt2.get() == -7).all() and (jw2.get() == -7.0).all()
            # nEntityTopicDistributions
            groups = groups_of(D, None)
            moff = np.concatenate([[0], np.cumsum([len(x) for x in groups])]).astype(np.int64)
            mem = np.concatenate([np.asarray(x, np.int64) for x in groups])
            want = smp.entity_topic_distributions(W3, 0.03, groups, -1, 5)
            jo = jvm.doubles(len(groups) * K)
            jvm.call("nEntityTopicDistributions", h, jvm.doubles(W3), 0.03, -1, 5, jvm.longs(moff), jvm.longs(mem), jo)
            assert jo.get().tobytes() == want.tobytes()
            # nSimilarPairs on those rows
            x = want[:D + 3]
            wi, wj, wv, wst = smp.similar_pairs(x, sn.COS_FOLDED, 0.15, min_weight=0.03)
            jx = jvm.doubles(x.ravel())
            jst, jmg = jvm.longs(5), jvm.doubles(1)
            n = jvm.call("nSimilarPairs", h, sn.COS_FOLDED, x.shape[0], K, jx, 0.03, 0.15, 0, 0, None, None, None, jst, jmg)
            assert n == len(wi) > 0
            ji, jj, js = jvm.ints(n), jvm.ints(n), jvm.doubles(n)
            assert jvm.call("nSimilarPairs", h, sn.COS_FOLDED, x.shape[0], K, jx, 0.03, 0.15, 0, 0, ji, jj, js, jst, jmg) == n
            assert np.array_equal(ji.get(), wi) and np.array_equal(jj.get(), wj) and js.get().tobytes() == wv.tobytes()
            assert list(jst.get()) == [wst.pairs_screened, wst.candidates, wst.emitted, wst.stripes, wst.regrown] and jmg.get()[0] == wst.margin
            ji2 = jvm.ints([-7])
            assert jvm.call("nSimilarPairs", h, sn.COS_FOLDED, x.shape[0], K, jx, 0.03, 0.15, 0, 0, ji2, jvm.ints(1), jvm.doubles(1), None, None) == n
            assert ji2.get()[0] == -7
            # a wrong array length is refused before the library is reached (mvhdp_last_error still holds the previous call's text)
            def refused(name, *args):
                with pytest.raises(H.JavaException) as e:
                    jvm.call(name, *args)
                assert e.value.cls == IAE, e.value
            refused("nSimilarPairs", h, sn.COS, x.shape[0], K, jvm.doubles(x.size - 1), 0.03, 0.15, 0, 0, None, None, None, None, None)
            refused("nSimilarPairs", h, sn.COS, x.shape[0], K, jvm.doubles(x.size + 1), 0.03, 0.15, 0, 0, None, None, None, None, None)
            refused("nSimilarPairs", h, sn.COS, x.shape[0], K, jx, 0.03, 0.15, 0, 0, jvm.ints(4), jvm.ints(5), jvm.doubles(4), None, None)
            refused("nSimilarPairs", h, sn.COS, x.shape[0], K, jx, 0.03, 0.15, 0, 0, jvm.ints(4), jvm.ints(4), jvm.doubles(3), None, None)
            refused("nSimilarPairs", h, sn.COS, x.shape[0], K, jx, 0.03, 0.15, 0, 0, None, None, None, jvm.longs(4), None)
            refused("nSimilarPairs", h, sn.COS, 1 << 20, 1 << 20, jx, 0.03, 0.15, 0, 0, None, None, None, None, None)   # the product as a jlong
            refused("nDocTopicsTop", h, jvm.doubles(M + 1), 0, D, 0.03, 3, None, None, None)
            refused("nDocTopicsTop", h, jvm.doubles(W3), 0, D, 0.03, 3, jvm.longs(D), None, None)
            refused("nDocTopicsTop", h, jvm.doubles(W3), 0, D + 1, 0.03, 3, None, None, None)
            refused("nDocTopicsTop", h, jvm.doubles(W3), 0, D, 0.03, 3, None, jvm.ints(3), jvm.doubles(4))
            refused("nEntityTopicDistributions", h, jvm.doubles(W3), 0.03, -1, 5, jvm.longs(moff), jvm.longs(mem), jvm.doubles(len(groups) * K - 1))
            refused("nEntityTopicDistributions", h, jvm.doubles(W3), 0.03, -1, 5, jvm.longs(moff), jvm.longs(mem[:-1]), jo)
            refused("nEntityTopicDistributions", h, jvm.doubles(M - 1), 0.03, -1, 5, jvm.longs(moff), jvm.longs(mem), jo)
            # a library error becomes a RuntimeException
            with pytest.raises(H.JavaException) as e:
                jvm.call("nSimilarPairs", h, sn.COS, x.shape[0], K, jx, 0.03, -1.0, 0, 0, None, None, None, None, None)
            assert e.value.cls == "java/lang/RuntimeException" and "threshold" in e.value.msg
        finally:
            j.close()
        for closed in (j.handle, h):                                         # a closed sampler: its handle is 0; and the jlong it had is refused too
            for name, args in (("nSimilarPairs", (sn.COS, x.shape[0], K, jx, 0.03, 0.15, 0, 0, None, None, None, None, None)),
                               ("nDocTopicsTop", (jvm.doubles(W3), 0, D, 0.03, 3, None, None, None)),
                               ("nEntityTopicDistributions", (jvm.doubles(W3), 0.03, -1, 5, jvm.longs(moff), jvm.longs(mem), jo))):
                with pytest.raises(H.JavaException) as e:
                    jvm.call(name, closed, *args)
                assert e.value.cls == "java/lang/IllegalStateException" and e.value.msg == "NativeSampler is closed"
        assert j.handle == 0 and h != 0
