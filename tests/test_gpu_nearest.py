"""mvhdp_nearest_entities and mvhdp_topic_top_entities on a device against tests/nearest_numpy.py: every id, count and value bit equal.

The candidate rows of the contract are the handle's own proportions, so the restatement is applied to what mvhdp_doc_topic_proportions
returns for the same handle; rows with chosen contents come from a one-view model whose entity d holds counts[d][k] tokens of topic k
(alpha = 0: theta_d is counts[d] / (len_d + alpha_sum), one division per entry).  The screen is held to its contract -- it never decides
-- by forcing every block, stripe and capacity border through the three knobs, and by the condition that it does screen."""
import ctypes as C

import numpy as np
import pytest

from mvtopicmodel_amd import NativeSampler, _lib
from mvtopicmodel_amd.native import SWEEP_LIVE, Hyper, NativeGroup, nearest_probe
from tests import nearest_numpy as nn
from tests import xview_cases as xc
from tests.helpers import INV, STATE, golden_sampler

pytestmark = pytest.mark.gpu
W1 = np.array([1.0])
KS, CS, NQS = [1, 2, 33, 100, 400], [1, 127, 128, 129, 300], [1, 64, 130]


def rows_model(counts, alpha=None, alpha_sum=1.0):
    """a one-view sampler whose entity d holds counts[d][k] tokens of topic k (type k); alpha [K] (default 0)"""
    counts = np.asarray(counts, dtype=np.int64)
    D, K = counts.shape
    tok = np.concatenate([np.repeat(np.arange(K, dtype=np.int32), counts[d]) for d in range(D)] + [np.zeros(0, np.int32)]).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(counts.sum(1))]).astype(np.int64)
    hy = Hyper.defaults(K, [K])
    hy.alpha[:, :K] = 0.0 if alpha is None else np.asarray(alpha, dtype=np.float64)
    hy.alpha_sum[:] = alpha_sum
    s = NativeSampler(K, [K])
    s.set_corpus(0, off, tok)
    s.set_view_presence(0, np.ones(D, dtype=np.uint8))       # an entity without tokens has the view, empty: nothing is carried over to it
    s.set_assignments(0, tok)
    s.set_hyper(hy)
    s.build_counts()
    return s


def random_counts(D, K, seed):
    rng = np.random.default_rng(seed)
    c = np.where(rng.random((D, K)) < min(1.0, 4.0 / K), rng.integers(1, 6, (D, K)), 0)
    c[np.arange(D), rng.integers(0, K, D)] += 1
    return c


def same(got, want, what):
    assert np.array_equal(got.counts, want[2]), (what, np.flatnonzero(got.counts != want[2])[:8])
    assert np.array_equal(got.ids, want[0]), (what, np.argwhere(got.ids != want[0])[:8])
    assert got.sims.dtype == np.float64 and got.sims.tobytes() == want[1].tobytes(), (what, np.argwhere(got.sims != want[1])[:8])


def check_stats(st, nq, nc, K, bq=0, sc=0):
    pr = nearest_probe(nq, nc, K, bq, sc)
    assert (st.cells_screened, st.blocks, st.margin) == (pr.cells_screened, pr.blocks, pr.margin)


class Model:
    """a sampler, its proportions, and the restated cosines of all its pairs (computed once)"""

    def __init__(self, s, w=W1, min_weight=-np.inf, query_rows=None):
        self.s, self.w = s, w
        self.theta = s.doc_topic_proportions(w)
        self.all = nn.cosine_rect(self.theta[:query_rows], self.theta, min_weight)   # handle-form queries come from the first query_rows entities

    def handle_form(self, n, q0, q1, c0, c1, excl, what="", **knobs):
        sim, okq, okc = self.all
        m = (sim[q0:q1, c0:c1], okq[q0:q1], okc[c0:c1])
        want = nn.nearest(None, None, n, self_index=(np.arange(q0, q1) - c0) if excl else None, id_base=c0, matrix=m)
        got = self.s.nearest_entities(self.w, n, q0=q0, q1=q1, c0=c0, c1=c1, exclude_self=excl, **knobs)
        same(got, want, (what, "handle", n, q0, q1, c0, c1, excl, knobs))
        return got

    def host_form(self, queries, n, c0=0, c1=None, min_weight=-np.inf, what="", matrix=None, **knobs):
        c1 = self.s.D if c1 is None else c1
        want = nn.nearest(queries, self.theta[c0:c1], n, min_weight, id_base=c0, matrix=matrix)
        got = self.s.nearest_entities(self.w, n, queries=queries, c0=c0, c1=c1, min_weight=min_weight, **knobs)
        same(got, want, (what, "host", n, c0, c1, knobs))
        return got


@pytest.mark.parametrize("K", KS)
def test_shapes_equal_the_restatement_bit_for_bit(K):
    rng = np.random.default_rng(K)
    for Cn in CS:
        alpha = rng.uniform(0.05, 0.15, K)
        with rows_model(random_counts(Cn, K, 100 * K + Cn), alpha, alpha.sum() * 1.25) as s:
            m = Model(s)
            for nq in NQS:
                q = rng.dirichlet(np.full(K, 0.3), nq)
                q[::3] = m.theta[rng.integers(0, Cn, len(q[::3]))]           # a share of the queries are rows of the corpus
                mat = nn.cosine_rect(q, m.theta)
                for n in sorted({1, 5, 20, Cn, Cn + 3}):
                    got = m.host_form(q, n, what=(K, Cn, nq), matrix=mat)
                    check_stats(got.stats, nq, Cn, K)
                    assert got.stats.regrown == 0 and got.stats.exact_only_rows == 0
            for n in sorted({1, 5, 20, Cn, Cn + 3}):
                for excl in (True, False):
                    got = m.handle_form(n, 0, Cn, 0, Cn, excl, what=(K, Cn))
                    assert (got.counts == min(n, Cn - (1 if excl else 0))).all()
            if Cn > 100:                                                     # windows: queries and candidates that overlap in part
                m.handle_form(5, 3, 90, 60, Cn - 1, True, what="window")
                m.handle_form(5, 64, Cn, 0, 70, False, what="window")
                m.host_form(m.theta[:7], 5, 60, Cn - 1, what="window")


@pytest.fixture(scope="module")
def m33():
    K, Cn = 33, 300
    alpha = np.random.default_rng(5).uniform(0.05, 0.15, K)
    s = rows_model(random_counts(Cn, K, 77), alpha, alpha.sum() * 1.25)
    yield Model(s)
    s.close()


def test_a_host_query_that_is_a_row_of_the_handle_and_one_an_ulp_off(m33):
    m = m33
    rows = [0, 17, 128, 299]
    own = m.handle_form(20, 0, 300, 0, 300, False)
    got = m.host_form(m.theta[rows], 20)
    for i, r in enumerate(rows):
        assert np.array_equal(got.ids[i], own.ids[r]) and got.sims[i].tobytes() == own.sims[r].tobytes()
    off = m.theta[rows].copy()
    for i in range(len(rows)):
        k = int(np.argmax(off[i]))
        off[i, k] = np.nextafter(off[i, k], 1.0 if i % 2 else 0.0)
    moved = m.host_form(off, 20)                                             # equal to the restatement for THAT row ...
    assert any(moved.sims[i].tobytes() != got.sims[i].tobytes() for i in range(len(rows)))   # ... which is not the row of the handle


def test_every_block_stripe_and_capacity_border(m33):
    m = m33
    q = np.random.default_rng(9).dirichlet(np.full(33, 0.3), 130)
    base = m.host_form(q, 20)
    for bq, sc in ((1, 0), (7, 50), (64, 127), (128, 128), (129, 129), (0, 1), (130, 299), (33, 300)):
        got = m.host_form(q, 20, block_queries=bq, stripe_candidates=sc, what="borders")
        check_stats(got.stats, 130, 300, 33, bq, sc)
        assert got.stats.candidates >= base.stats.candidates and got.stats.regrown == 0
        if sc == 0 or sc >= 300:
            assert got.stats.candidates == base.stats.candidates           # one stripe: the cut is the n-th largest screen value itself
        m.handle_form(5, 10, 140, 0, 300, True, block_queries=bq, stripe_candidates=sc, what="borders")
    small = m.host_form(q, 20, block_queries=64, stripe_candidates=96, candidate_capacity=8, what="regrow")
    assert small.stats.regrown >= 1
    assert small.stats.candidates == m.host_form(q, 20, block_queries=64, stripe_candidates=96).stats.candidates
    exact = m.host_form(q, 20, candidate_capacity=base.stats.candidates)    # exactly enough
    assert exact.stats.regrown == 0
    assert m.host_form(q, 20, candidate_capacity=base.stats.candidates - 1).stats.regrown == 1


def test_duplicate_rows_straddling_the_nth_place():
    K, Cn, n = 33, 300, 20
    rng = np.random.default_rng(21)
    counts = random_counts(Cn, K, 21)
    v = rng.integers(1, 9, K)
    for d in (3, 70, 131, 260, 299):
        counts[d] = v                                                        # five rows along the query
    dup = v.copy(); dup[4] += 1
    copies = np.r_[40:60, 190:210]                                           # forty equal rows, across a tile border
    counts[copies] = dup
    with rows_model(counts) as s:
        m = Model(s)
        q = v[None, :].astype(np.float64)
        sim = nn.cosine_rect(q, m.theta)[0][0]
        assert len(set(sim[copies])) == 1 and (sim[[3, 70, 131, 260, 299]] > sim[40]).all() and (np.delete(sim, np.r_[copies, [3, 70, 131, 260, 299]]) < sim[40]).all()
        got = m.host_form(q, n, candidate_capacity=16, what="duplicates")
        assert list(got.ids[0, 5:]) == list(copies[:15])                     # id order among equals
        assert got.stats.regrown >= 1 and got.stats.candidates >= 45         # every copy is a candidate: the block asked for more room
        m.host_form(q, n, candidate_capacity=16, stripe_candidates=45, what="duplicates in stripes")
        h = m.handle_form(n, 40, 60, 0, Cn, True, candidate_capacity=16, what="duplicates, handle form")
        assert all(list(h.ids[i, :n]) == [c for c in copies if c != 40 + i][:n] for i in range(20))


def test_near_ties_at_the_nth_place_are_decided_by_the_exact_stage():
    """Rows along one direction with different lengths: theta differs by a rounding per entry, so the exact cosines against a query lie an
    ulp or two apart while the fp32 screens are equal or the other way round.  Wherever the n-th and (n + 1)-th place are such a pair the
    list must still be the restatement's."""
    K = 33
    rng = np.random.default_rng(4)
    counts = random_counts(300, K, 4)
    v = rng.integers(1, 7, K)
    along = [7, 90, 128, 200, 255, 299]
    for i, d in enumerate(along):
        counts[d] = v * (i + 1)
    with rows_model(counts) as s:
        m = Model(s)
        q = (v + rng.random(K) * 1e-3)[None, :]
        sim = nn.cosine_rect(q, m.theta)[0][0]
        scr = nn.screen_f32_rect(q, m.theta[along])[0]
        order = nn.first_n(sim, np.arange(300), 300)
        assert set(order[:6]) == set(along)
        decided = 0
        for n in range(1, 6):
            a, b = order[n - 1], order[n]
            if sim[a] != sim[b] and abs(sim[a] - sim[b]) <= 4 * np.spacing(sim[a]) and scr[along.index(a)] <= scr[along.index(b)]:
                decided += 1
            got = m.host_form(q, n, what="near ties")
            assert list(got.ids[0]) == list(order[:n])
            m.host_form(q, n, stripe_candidates=100, block_queries=1, what="near ties in stripes")
        assert decided >= 1, "the fixture has no near-tie that the screen cannot decide: reseed"


def wild_rows(x):
    with np.errstate(all="ignore"):
        a = np.abs(x)
        n = nn.sn.norms(x)
        return ((x != 0) & ~((a >= 2.0 ** -500) & (a <= 2.0 ** 500))).any(1) & (n > 0) & np.isfinite(n)


def test_degenerate_rows():
    K, Cn = 33, 140
    counts = random_counts(Cn, K, 8)
    counts[5] = 0                                                            # no tokens: a zero row
    counts[:, 2] = 0
    counts[::4, 2] = 3                                                       # a quarter of the entities hold topic 2 ...
    alpha = np.zeros(K); alpha[2] = 2.0 ** -600                              # ... the others an entry of 2^-600 / (len + 1) there: not screened
    with rows_model(counts, alpha) as s:
        m = Model(s)
        wild_c = wild_rows(m.theta)
        listable = int(m.all[2].sum())
        assert not m.all[2][5] and 0 < wild_c.sum() < listable and not wild_c[0] and m.all[2][0]
        rng = np.random.default_rng(8)
        q = rng.dirichlet(np.full(K, 0.3), 9)
        q[1] = 0.0                                                           # zero norm
        q[2, 3] = np.nan                                                     # NaN norm
        q[3] = q[3] * 2.0 ** 505                                             # entries beyond 2^500, a finite norm: not screened
        q[4, 0] = 2.0 ** 600                                                 # the norm overflows: lists nothing
        q[6] = q[6] * 2.0 ** -510
        assert list(wild_rows(q)) == [False, False, False, True, False, False, True, False, False]
        for n in (1, 5, Cn):
            got = m.host_form(q, n, what="degenerate")
            assert list(got.counts[[1, 2, 4]]) == [0, 0, 0] and not (got.ids == 5).any()
            assert got.stats.exact_only_rows == int(wild_c.sum()) + 2
            assert got.counts[3] == got.counts[6] == min(n, listable)
            got = m.handle_form(n, 0, Cn, 0, Cn, True, what="degenerate")
            assert got.counts[5] == 0 and got.stats.exact_only_rows == 2 * int(wild_c.sum())
            m.handle_form(n, 0, Cn, 0, Cn, True, block_queries=50, stripe_candidates=33, what="degenerate, cut")
        got = m.host_form(q, 5, min_weight=0.02, what="min_weight")         # the filter empties the tiny entries: nothing is wild any more
        assert got.stats.exact_only_rows == 1 and got.counts[6] == 0
    alpha = np.zeros(K); alpha[2] = 2.0 ** 600                               # every candidate's norm overflows
    with rows_model(counts[:20], alpha) as s:
        got = Model(s).host_form(q, 5, what="overflow")
        assert (got.counts == 0).all() and got.stats.candidates == 0
    alpha = np.zeros(K); alpha[2] = 2.0 ** 509                               # every candidate is beyond the screen, and finite
    with rows_model(counts[:20], alpha) as s:
        got = Model(s).host_form(q, 5, what="all wild")
        assert got.stats.exact_only_rows == 20 + 2 and got.stats.candidates == 20 * 6


def test_missing_views_inactive_topics_and_a_live_sweep():
    inactive = np.zeros(64, dtype=np.uint8)
    inactive[[0, 17, 63]] = 1
    for c in (xc.make(100, 128, 65, 3), xc.make(64, 127, 65, 3, inactive=inactive)):
        assert any((np.diff(c.doc_off[v]) == 0).any() for v in range(c.M))   # entities without a view are in
        s = NativeSampler(c.K, c.V)
        with s:
            for v in range(c.M):
                s.set_corpus(v, c.doc_off[v], c.tokens[v])
                s.set_assignments(v, c.z[v])
            s.set_hyper(c.hy)
            s.build_counts()
            for w in (c.weights, np.array([1.0, 0.7, 0.4])):
                m = Model(s, w)
                m.handle_form(20, 0, c.D, 0, c.D, True, what="carry-over")
                m.host_form(m.theta[::5] * 3.0, 5, what="carry-over")
            if c.hy.inactive is None:
                before = m.theta.copy()
                s.sweep(0, 11, flags=SWEEP_LIVE)
                m = Model(s, np.array([1.0, 0.7, 0.4]))
                assert (m.theta != before).any()
                m.handle_form(20, 0, c.D, 0, c.D, True, what="after a live sweep")


def test_the_sims_are_those_of_similar_pairs(m33):
    m = m33
    i, j, v, _ = m.s.similar_pairs(m.theta, "cos", 0.0)
    pair = {(int(a), int(b)): x for a, b, x in zip(i, j, v)}
    assert len(pair) == 300 * 299 // 2                                       # positive rows: every pair is above 0
    got = m.handle_form(20, 0, 300, 0, 300, True)
    for q in range(300):
        for c, x in zip(got.ids[q], got.sims[q]):
            assert np.float64(x).tobytes() == np.float64(pair[(min(q, int(c)), max(q, int(c)))]).tobytes()


@pytest.mark.parametrize("K", [33, 100, 400])
def test_the_screen_must_screen(K):
    """The seeded rows, as entities: candidate rows can only be a model's proportions, so entity d holds round(2000 x_d[k]) tokens of topic
    k and theta_d is x_d to 1 / 2000 per entry.  At most 2 n candidates per query: a condition, not a measurement."""
    for Cn in (300, 1000):
        x = np.random.default_rng(20261019).dirichlet(np.full(K, 0.1), Cn)
        counts = np.floor(x * 2000 + 0.5).astype(np.int64)
        with rows_model(counts) as s:
            m = Model(s, query_rows=64)
            for n in (5, 20):
                got = m.handle_form(n, 0, 64, 0, Cn, True, what=("screen", K, Cn, n))
                print(f"K={K} C={Cn} n={n}: candidates {got.stats.candidates} for 64 queries, margin {got.stats.margin:.3e}")
                assert got.stats.candidates <= 2 * n * 64
                assert got.stats.candidates >= n * 64 and got.stats.exact_only_rows == 0


# ---- top entities per topic ------------------------------------------------------------------------------------------------------------
def same_top(got, want, what):
    assert np.array_equal(got[2], want[2]), (what, got[2], want[2])
    assert np.array_equal(got[0], want[0]), (what, np.argwhere(got[0] != want[0])[:8])
    assert got[1].tobytes() == want[1].tobytes(), what


@pytest.mark.parametrize("K", [1, 20, 400])
def test_topic_top_entities_shapes_ties_threshold_and_chunk_borders(K):
    for D in (1, 65, 300):
        counts = random_counts(D, K, 7 * K + D)
        if D > 40:
            counts[30:40] = counts[3]                                        # identical entities: ties in every topic
        alpha = np.random.default_rng(D).uniform(0.05, 0.15, K)
        with rows_model(counts, alpha, alpha.sum() * 1.25) as s:
            prop = s.doc_topic_proportions(W1)
            thr = float(np.sort(prop.max(1))[D // 2])                        # a weight of the matrix itself: strictly above
            for n in sorted({1, 7, D + 1}):
                for t in (-np.inf, thr, 2.0):
                    want = nn.topic_top_entities(prop, n, t)
                    got = s.topic_top_entities(W1, n, t)
                    same_top(got, want, (K, D, n, t))
                    assert got[0].tobytes() == s.topic_top_entities(W1, n, t)[0].tobytes()
                    for ce, se in ((7, 3), (64, 5), (0, 64), (65, 64)) + (((1, 0), (0, 1)) if n <= 7 else ()):
                        same_top(s.topic_top_entities(W1, n, t, chunk_entities=ce, slice_entities=se), want, (K, D, n, t, ce, se))
            if D > 40:
                same_top(s.topic_top_entities(W1, 7, -np.inf, 20, 50, chunk_entities=7), nn.topic_top_entities(prop[20:50], 7, id_base=20), "window")
                assert (s.topic_top_entities(W1, 3, d0=9, d1=9)[2] == 0).all()


@pytest.mark.parametrize("name", ["m3_k20", "m3_k100_inactive"])
def test_both_entry_points_on_the_goldens(name):
    w = np.array([1.0, 0.7, 0.4])
    with golden_sampler(name)[0] as s:
        prop = s.doc_topic_proportions(w)
        for n, t in ((1, -np.inf), (20, -np.inf), (20, 0.03), (s.D + 1, 0.03)):
            same_top(s.topic_top_entities(w, n, t), nn.topic_top_entities(prop, n, t), (name, n, t))
            same_top(s.topic_top_entities(w, n, t, chunk_entities=11, slice_entities=4), nn.topic_top_entities(prop, n, t), (name, n, t, "cut"))
        m = Model(s, w)
        m.handle_form(20, 0, s.D, 0, s.D, True, what=name)
        m = Model(s, w, min_weight=0.03)
        got = s.nearest_entities(w, 20, min_weight=0.03)
        same(got, nn.nearest(None, None, 20, self_index=np.arange(s.D), matrix=m.all), (name, "min_weight"))


def test_a_group_of_two_members_equals_one_handle():
    c = xc.make(100, 128, 65, 3)
    lens = [np.diff(c.doc_off[v]) for v in range(c.M)]
    cut = next(d for d in range(c.D // 2, c.D) if all(l[d] > 0 for l in lens))   # the second member's first entity has every view: nothing to carry over
    w = np.array([1.0, 0.7, 0.4])

    def load(lo, hi):
        s = NativeSampler(c.K, c.V)
        for v in range(c.M):
            off = c.doc_off[v]
            s.set_corpus(v, off[lo:hi + 1] - off[lo], c.tokens[v][off[lo]:off[hi]])
            s.set_assignments(v, c.z[v][off[lo]:off[hi]])
        s.set_hyper(c.hy)
        s.build_counts()
        return s
    one, members = load(0, c.D), [load(0, cut), load(cut, c.D)]
    try:
        g = NativeGroup.__new__(NativeGroup)                                 # (no collective is needed for this: the local members, as predict_items)
        g.members, g.g = members, None
        q = np.random.default_rng(2).dirichlet(np.full(c.K, 0.3), 40)
        q[:5] = one.doc_topic_proportions(w)[[0, cut - 1, cut, cut + 1, c.D - 1]]
        for n in (1, 20, c.D + 2):
            a, b = one.nearest_entities(w, n, queries=q), g.nearest_entities(w, n, q)
            assert np.array_equal(a.ids, b.ids) and a.sims.tobytes() == b.sims.tobytes() and np.array_equal(a.counts, b.counts)
            assert b.stats.candidates >= a.stats.candidates and b.stats.blocks == 2
            for t in (-np.inf, 0.05):
                same_top(g.topic_top_entities(w, n, t), one.topic_top_entities(w, n, t), ("group", n, t))
        same_top(g.topic_top_entities(w, 7, 0.01, chunk_entities=9), one.topic_top_entities(w, 7, 0.01), "group, cut")
    finally:
        for s in [one] + members:
            s.close()


def test_error_paths_leave_every_output_untouched(m33):
    s, K, D = m33.s, 33, 300
    L = s.L
    w = np.ascontiguousarray(W1)
    q = np.ascontiguousarray(m33.theta[:4])
    ids, sims, counts = np.full((4, 3), -7, np.int64), np.full((4, 3), -7.0), np.full(4, -7, np.int32)
    st = _lib.NearestStatsC()

    def args(**kw):
        d = dict(view_weights=w.ctypes.data, c0=0, c1=D, queries=q.ctypes.data, nq=4, q0=0, q1=0, exclude_self=0, n=3, min_weight=-np.inf,
                 block_queries=0, stripe_candidates=0, candidate_capacity=0)
        d.update(kw)
        return _lib.NearestArgsC(**d)

    def call(a, i=ids, v=sims, c=counts):
        p = lambda x: None if x is None else x.ctypes.data
        return L.mvhdp_nearest_entities(s.h, None if a is None else C.byref(a), p(i), p(v), p(c), C.byref(st))
    bad = [None, args(view_weights=None), args(n=0), args(n=-1), args(c0=-1), args(c1=D + 1), args(c0=5, c1=4), args(nq=-1),
           args(queries=None, q0=-1, q1=4), args(queries=None, q0=0, q1=D + 1), args(queries=None, q0=5, q1=4), args(min_weight=np.nan),
           args(block_queries=-1), args(stripe_candidates=-1), args(candidate_capacity=-1)]
    for a in bad:
        assert call(a) == INV
    assert call(args(), i=None) == INV and call(args(), v=None) == INV and call(args(), c=None) == INV
    assert b"nearest_entities" in L.mvhdp_last_error(s.h)
    assert (ids == -7).all() and (sims == -7.0).all() and (counts == -7).all()
    assert call(args()) == 0 and (counts == 3).all() and (ids >= 0).all()    # and the good call writes all of them
    assert call(args(nq=0)) == 0 and st.blocks == 0
    e_ids, e_counts = np.full((4, 3), -7, np.int64), np.full(4, -7, np.int32)
    assert call(args(c0=7, c1=7), i=e_ids, c=e_counts) == 0 and (e_ids == -1).all() and (e_counts == 0).all()
    tid, tw, tc = np.full((K, 2), -7, np.int64), np.full((K, 2), -7.0), np.full(K, -7, np.int32)
    top = lambda wp, d0, d1, n, t, ce, se, i=tid, v=tw, c=tc: L.mvhdp_topic_top_entities(
        s.h, wp, d0, d1, n, t, ce, se, None if i is None else i.ctypes.data, None if v is None else v.ctypes.data, None if c is None else c.ctypes.data)
    for a in ((None, 0, D, 2, 0.0, 0, 0), (w.ctypes.data, -1, D, 2, 0.0, 0, 0), (w.ctypes.data, 0, D + 1, 2, 0.0, 0, 0), (w.ctypes.data, 5, 4, 2, 0.0, 0, 0),
              (w.ctypes.data, 0, D, 0, 0.0, 0, 0), (w.ctypes.data, 0, D, 1025, 0.0, 0, 0), (w.ctypes.data, 0, D, 2, np.nan, 0, 0),
              (w.ctypes.data, 0, D, 2, 0.0, -1, 0), (w.ctypes.data, 0, D, 2, 0.0, 0, -1)):
        assert top(*a) == INV
    assert top(w.ctypes.data, 0, D, 2, 0.0, 0, 0, i=None) == INV and top(w.ctypes.data, 0, D, 2, 0.0, 0, 0, v=None) == INV
    assert top(w.ctypes.data, 0, D, 2, 0.0, 0, 0, c=None) == INV
    assert (tid == -7).all() and (tw == -7.0).all() and (tc == -7).all()
    assert top(w.ctypes.data, 0, D, 2, 0.0, 0, 0) == 0 and (tc == 2).all()
    # a handle with a corpus and no hyper-parameters: MVHDP_ERR_STATE, nothing written
    with NativeSampler(4, [8]) as bare:
        bare.set_corpus(0, np.array([0, 2, 3], np.int64), np.array([1, 2, 3], np.int32))
        i2, v2, c2 = np.full((2, 1), -7, np.int64), np.full((2, 1), -7.0), np.full(2, -7, np.int32)
        a = _lib.NearestArgsC(w.ctypes.data, 0, 2, None, 0, 0, 2, 0, 1, -np.inf, 0, 0, 0)
        assert L.mvhdp_nearest_entities(bare.h, C.byref(a), i2.ctypes.data, v2.ctypes.data, c2.ctypes.data, None) == STATE
        t4 = np.full((4, 1), -7, np.int64)
        assert L.mvhdp_topic_top_entities(bare.h, w.ctypes.data, 0, 2, 1, 0.0, 0, 0, t4.ctypes.data, np.zeros((4, 1)).ctypes.data, np.zeros(4, np.int32).ctypes.data) == STATE
        assert (i2 == -7).all() and (c2 == -7).all() and (t4 == -7).all()
