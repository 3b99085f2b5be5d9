"""mvhdp_predict_entities / mvhdp_rank_entities on a device against the sequential restatement of their contract
(tests/native/xview_entities_ref.c): ids, counts and ranks equal, every score bit for bit.  theta is what mvhdp_doc_topic_proportions
returns for the same handle (the contract says so); phi, psi and the chains are the restatement's own.  The comparison target is the
restatement, never the device's output.  Shapes (tests/xview_entities_cases.py): K below, at and above the 16-topic slab; queries and
candidates below, at and above the 64 x 128 tile; blocks of 128 entities and 64 queries forced, so that a top n is carried over at
least three blocks; a candidate range longer than the selection's LDS; ties across the n-th place and a block border.  No tolerance
anywhere: integers and exact fp64 values decide everything."""
import ctypes as C

import numpy as np
import pytest

from mvtopicmodel_amd import MvhdpError, NativeSampler, _lib
from mvtopicmodel_amd.native import SWEEP_LIVE, SWEEP_NO_APPLY, NativeGroup
from tests import xview_cases as xc
from tests import xview_entities_cases as ec
from tests import xview_entities_ref as er
from tests import xview_ref as xr
from tests.helpers import INV, STATE, bits, load

pytestmark = pytest.mark.gpu
FORCED = dict(block_entities=128, block_queries=64)


class Ref:
    """the restatement's scores [nq][c1 - c0] and excluded cells of one query set over one candidate range (computed once)"""

    def __init__(self, x, items=None, weights=None, psi=None, c0=0, c1=None):
        c = x.c
        self.x, self.items, self.weights, self.c0, self.c1 = x, items, weights, c0, c.D if c1 is None else c1
        self.host_psi = psi
        self.psi = psi if psi is not None else er.psi_rows(x.nwk, x.nk, c.hy.beta[c.m], c.hy.beta_sum[c.m], c.hy.inactive, items, weights)
        self.S = er.scores(x.theta[self.c0:self.c1], self.psi)
        self.ex = None
        if psi is None:
            off, tok = c.doc_off[c.m], c.tokens[c.m]
            self.ex = er.excluded(off[self.c0:self.c1 + 1], tok[off[self.c0]:off[self.c1]], items)

    def call(self, n, excl=True, **knobs):
        x = self.x
        return x.s.predict_entities(x.c.m, x.weights, n, items=None if self.host_psi is not None else self.items, weights=None if self.host_psi is not None else self.weights,
                                    psi=self.host_psi, c0=self.c0, c1=self.c1, exclude_present=excl, **knobs)

    def check_predict(self, n, excl=True, what="", **knobs):
        ex = self.ex if excl else None
        want = er.predict(self.S, n, ex, id0=self.c0)
        got = self.call(n, excl, **knobs)
        assert got.ids.dtype == np.int64 and got.scores.dtype == np.float64 and got.counts.dtype == np.int32
        assert np.array_equal(got.counts, want[2]), (what, n, knobs, np.flatnonzero(got.counts != want[2])[:8])
        assert np.array_equal(got.ids, want[0]), (what, n, knobs, np.argwhere(got.ids != want[0])[:8])
        assert np.array_equal(bits(got.scores), bits(want[1])), (what, n, knobs)
        assert got.stats.cells == self.S.size and got.stats.excluded == (0 if ex is None else int(ex.sum())) and got.stats.blocks >= 1
        return got

    def check_rank(self, query, entity, excl=True, what="", **knobs):
        x = self.x
        ex = self.ex if excl else None
        want = er.rank(self.S, query, np.asarray(entity) - self.c0, ex)
        got = x.s.rank_entities(x.c.m, x.weights, query, entity, items=None if self.host_psi is not None else self.items,
                                weights=None if self.host_psi is not None else self.weights, psi=self.host_psi, c0=self.c0, c1=self.c1, exclude_present=excl, **knobs)
        assert got.rank.dtype == np.int64
        assert np.array_equal(bits(got.score), bits(want[0])), (what, knobs, np.flatnonzero(got.score != want[0])[:8])
        assert np.array_equal(got.rank, want[1]), (what, knobs, np.flatnonzero(got.rank != want[1])[:8])
        return got


class Loaded:
    """the case in a sampler, with the sampler's own theta and counts"""

    def __init__(self, c, weights=None):
        self.c, self.s = c, load(c)
        self.weights = c.weights if weights is None else np.asarray(weights, dtype=np.float64)
        self.refresh()

    def refresh(self):
        self.nwk, self.nk = self.s.get_counts(self.c.m)
        self.theta = self.s.doc_topic_proportions(self.weights)


@pytest.fixture(scope="module")
def loaded():
    made = {}

    def get(K):
        if K not in made:
            made[K] = Loaded(ec.make(K))
        return made[K]
    yield get
    for x in made.values():
        x.s.close()


@pytest.mark.parametrize("shape", ec.SHAPES, ids=str)
def test_shapes_equal_the_restatement(loaded, shape):
    K, nq, Cn = shape
    x = loaded(K)
    c = x.c
    if c.no_source >= 0:                                                     # the carry-over is in play: the proportions of the entity in front
        assert np.array_equal(x.theta[c.no_source], x.theta[c.no_source - 1])
    c0 = min(7, c.D - Cn)
    items, weights = ec.queries(c, nq, seed=K)
    r = Ref(x, items, weights, c0=c0, c1=c0 + Cn)
    assert nq < 3 or Cn < 100 or (r.ex.sum(1) > 0).sum() > 1                 # exclusion has something to decide
    for n in (1, 2, 20, Cn + 3):
        r.check_predict(n, True, what=shape, **FORCED)
    r.check_predict(20, True, what=shape)
    r.check_predict(20, False, what=shape, **FORCED)
    q, e = ec.pairs(c, nq, c0, c0 + Cn, 60, items, seed=K)
    got = r.check_rank(q, e, True, what=shape, **FORCED)
    r.check_rank(q, e, False, what=shape)
    assert 0.0 < got.mrr() <= 1.0 and got.mrr() == float(np.mean(1.0 / (got.rank + 1.0)))
    h = Ref(x, psi=r.psi, c0=c0, c1=c0 + Cn)                                 # the same rows from the host: the same lists, nothing excluded
    h.check_predict(20, True, what=shape, **FORCED)
    h.check_rank(q, e, True, what=shape)


def test_one_item_queries_as_a_1d_array_and_an_unweighted_set(loaded):
    x = loaded(17)
    V = x.c.V[x.c.m]
    r = Ref(x, np.arange(V, dtype=np.int32))                                 # every type of the view: psi is the phi table
    assert np.array_equal(bits(r.psi), bits(xr.phi_table(x.nwk, x.nk, x.c.hy.beta[x.c.m], x.c.hy.beta_sum[x.c.m], x.c.hy.inactive)))
    r.check_predict(20, True, what="1-D", **FORCED)
    r.check_predict(20, True, what="1-D")
    u = Ref(x, [[3, 9, 3], [5], []])                                         # without weights every weight is 1.0
    u.check_predict(5, True, what="unweighted")


def test_1024_of_1100_candidates():
    x = Loaded(xc.make(5, 40, 1100, 3))
    try:
        items, weights = ec.queries(x.c, 3)
        r = Ref(x, items, weights)
        got = r.check_predict(1024, False, what="n = 1024", **FORCED)
        assert (got.counts == 1024).all()
        r.check_predict(1024, True, what="n = 1024")
        with pytest.raises(MvhdpError) as e:
            r.call(1025)
        assert e.value.code == INV and "1..1024" in str(e.value)
    finally:
        x.s.close()


def test_9000_candidates_the_selection_beyond_lds():
    """default knobs: blocks of 8192 entities, two of them; block_entities = 9000: one block whose row of keys does not fit the 64 KiB
    of LDS and is selected from memory.  Few topics and short documents: many equal scores, the entity id decides"""
    x = Loaded(xc.make(3, 30, 9000, 3))
    try:
        r = Ref(x, [[4], [7, 2, 7]], [[1.0], [0.5, 2.0, 1.0]])
        for n in (1, 20, 300):
            a = r.check_predict(n, True, what="9000")
            b = r.check_predict(n, True, what="9000 in one block", block_entities=9000)
            assert a.stats.blocks == 2 and b.stats.blocks == 1
        r.check_predict(20, False, what="9000", block_entities=9000)
        q = np.array([0, 1, 1, 0], dtype=np.int64)
        e = np.array([8999, 0, 8192, 8191], dtype=np.int64)
        r.check_rank(q, e, True, what="9000")
        r.check_rank(q, e, True, what="9000 in one block", block_entities=9000)
    finally:
        x.s.close()


def test_ties_across_the_nth_place_and_a_block_border():
    """40 entities [100, 140) with identical documents: identical theta, equal scores for every query; blocks of 128 entities cut the
    run, n is chosen (from the restatement's full list) so that the n-th place falls inside it"""
    c, template = ec.with_clones(ec.make(16), 100, 40)
    x = Loaded(c)
    try:
        assert all(np.array_equal(bits(x.theta[d]), bits(x.theta[template])) for d in range(100, 140))
        items, weights = ec.queries(c, 12)
        tested = 0
        for j in range(12):
            r = Ref(x, [items[j]], [weights[j]])
            for excl in (False, True):
                full = er.predict(r.S, c.D, r.ex if excl else None)
                listed = full[0][0, :full[2][0]].tolist()
                if 100 not in listed:
                    continue                                                 # the run holds an item of the query: excluded as one
                p = listed.index(100)
                assert listed[p:p + 40] == list(range(100, 140))
                n = p + 20
                # the condition the inputs must meet: equal scores really straddle the n-th place
                assert full[1][0, n - 1] == full[1][0, n] and listed[n - 1] == 119 and listed[n] == 120
                r.check_predict(n, excl, what=("ties", j), **FORCED)
                r.check_predict(n, excl, what=("ties", j))
                r.check_predict(n, excl, what=("ties", j), block_entities=110)          # the border at 110, the n-th place at 119 / 120
                got = r.check_rank(np.zeros(3, dtype=np.int64), np.array([100, 119, 139]), excl, what=("ties", j), **FORCED)
                assert got.rank[1] == got.rank[0] + 19 and got.rank[2] == got.rank[0] + 39
                tested += 1
        assert tested >= 6
    finally:
        x.s.close()


def test_a_host_psi_row_of_zeros_lists_the_first_candidates_by_id(loaded):
    """every score of the row is +0.0 and every key equal: nothing for the selection to descend on.  129 candidates in blocks of 128: the
    first block fills the carry (5 of 5), the second meets it full; blocks of 64 and of 3: the carry fills over two blocks"""
    x = loaded(17)
    c0, Cn = 7, 129                                                          # the smallest shape of ec.SHAPES that is cut into blocks
    items, weights = ec.queries(x.c, 3, seed=17)
    psi = Ref(x, items, weights, c0=c0, c1=c0 + Cn).psi.copy()
    psi[1] = 0.0
    h = Ref(x, psi=psi, c0=c0, c1=c0 + Cn)
    assert (bits(h.S[1]) == 0).all() and (h.S[0] > 0.0).all()
    for be in (128, 64, 3):
        got = h.check_predict(5, True, what=("zeros", be), block_entities=be, block_queries=64)
        assert got.counts[1] == 5 and got.ids[1].tolist() == list(range(c0, c0 + 5)) and (bits(got.scores[1]) == 0).all()
        assert got.stats.blocks == -(-Cn // be)


def test_a_host_psi_one_ulp_away_from_the_device_built_row(loaded):
    x = loaded(64)
    items, weights = ec.queries(x.c, 9)
    r = Ref(x, items, weights)
    psi = np.where(r.psi > 0.0, np.nextafter(r.psi, np.inf), r.psi)          # every entry that is not 0: the next double up
    h = Ref(x, psi=psi)
    assert (bits(h.S) != bits(r.S)).any()                                    # ... and the ulp is seen in the scores
    got = h.check_predict(20, True, what="ulp", **FORCED)
    same = Ref(x, psi=r.psi).check_predict(20, True, what="host rows")
    assert (bits(got.scores) != bits(same.scores)).any()
    q, e = ec.pairs(x.c, 9, 0, x.c.D, 40, items)
    h.check_rank(q, e, True, what="ulp")


def test_inactive_topics_and_a_weight_on_the_predicted_view():
    inactive = np.zeros(64, dtype=np.uint8)
    inactive[[0, 17, 63]] = 1
    x = Loaded(ec.make(64, inactive=inactive), weights=[1.0, 0.5, 0.7])      # view m takes part in theta here
    try:
        items, weights = ec.queries(x.c, 20)
        r = Ref(x, items, weights)
        assert (r.psi[:, [0, 17, 63]] == 0.0).all() and (r.psi[0] > 0.0).sum() == 61
        r.check_predict(20, True, what="inactive", **FORCED)
        r.check_predict(20, False, what="inactive")
        r.check_rank(*ec.pairs(x.c, 20, 0, x.c.D, 50, items), True, what="inactive")
        plain = er.scores(x.theta, er.psi_rows(x.nwk, x.nk, x.c.hy.beta[1], x.c.hy.beta_sum[1], None, items, weights))
        assert (plain != r.S)[[j for j in range(20) if items[j]]].mean() > 0.5           # ... and that is seen in the scores
        other = x.s.doc_topic_proportions(x.c.weights)
        assert (other != x.theta).any()                                      # ... as is the weight of view m
    finally:
        x.s.close()


def test_after_a_live_sweep_and_behind_a_no_apply_sweep():
    x = Loaded(ec.make(64, seed=1))
    s, c = x.s, x.c
    try:
        items, weights = ec.queries(c, 10)
        before = Ref(x, items, weights).S
        s.sweep(0, 11, flags=SWEEP_LIVE)
        x.refresh()
        r = Ref(x, items, weights)
        assert (r.S != before).any()
        r.check_predict(20, True, what="live", **FORCED)
        r.check_rank(*ec.pairs(c, 10, 0, c.D, 40, items), True, what="live")
        s.sweep(1, 11, flags=SWEEP_NO_APPLY)                                 # its deltas wait: the counts are not the model's
        for call in (lambda: r.call(5), lambda: s.rank_entities(c.m, x.weights, [0], [0], items=items),
                     lambda: s.predict_entities(c.m, x.weights, 5, psi=r.psi)):
            with pytest.raises(MvhdpError) as e:
                call()
            assert e.value.code == STATE and "pending" in str(e.value)
        s.apply_delta()
        x.refresh()
        Ref(x, items, weights).check_predict(20, True, what="applied")
        s.set_assignments(0, s.get_assignments(0))                           # assignments replaced: the counts are stale until recounted
        with pytest.raises(MvhdpError) as e:
            r.call(5)
        assert e.value.code == STATE
        s.build_counts()
        Ref(x, items, weights).check_predict(20, True, what="recounted")
    finally:
        s.close()


def test_one_item_queries_have_the_bits_of_score_items(loaded):
    x = loaded(100)
    c = x.c
    V = c.V[c.m]
    rng = np.random.default_rng(3)
    ent = rng.integers(0, c.D, 200).astype(np.int64)
    item = rng.integers(0, V, 200).astype(np.int32)
    theirs = x.s.score_items(c.m, x.weights, ent, item, exclude_present=False)
    ours = x.s.rank_entities(c.m, x.weights, item.astype(np.int64), ent, items=np.arange(V, dtype=np.int32), exclude_present=False, **FORCED)
    assert np.array_equal(bits(ours.score), bits(theirs.score))


def test_the_full_lists_of_both_sides_hold_the_same_scores():
    x = Loaded(xc.make(5, 3, 65, 3))
    try:
        c = x.c
        V, D = c.V[c.m], c.D
        items, sc, counts = x.s.predict_items(c.m, x.weights, V, exclude_present=False)
        by_entity = np.zeros((V, D)); by_entity[items.T, np.arange(D)[None, :]] = sc.T
        r = x.s.predict_entities(c.m, x.weights, D, items=np.arange(V, dtype=np.int32), exclude_present=False)
        assert (counts == V).all() and (r.counts == D).all()
        by_item = np.zeros((V, D)); by_item[np.arange(V)[:, None], r.ids] = r.scores
        assert np.array_equal(bits(by_item), bits(by_entity))
        # with exclusion the same cells are missing on both sides: entity d holds type w
        items, sc, counts = x.s.predict_items(c.m, x.weights, V, exclude_present=True)
        r = x.s.predict_entities(c.m, x.weights, D, items=np.arange(V, dtype=np.int32), exclude_present=True)
        listed_e = np.zeros((V, D), dtype=bool); listed_i = np.zeros((V, D), dtype=bool)
        for d in range(D):
            listed_e[items[d, :counts[d]], d] = True
        for w in range(V):
            listed_i[w, r.ids[w, :r.counts[w]]] = True
        assert np.array_equal(listed_e, listed_i) and not listed_i.all() and r.stats.excluded == int((~listed_i).sum())
    finally:
        x.s.close()


def test_a_group_of_two_members_equals_one_handle(loaded):
    x = loaded(100)
    c = x.c
    lens = [np.diff(c.doc_off[v]) for v in range(c.M)]
    cut = next(d for d in range(c.D // 2, c.D) if all(l[d] > 0 for l in lens))   # the second member's first entity has every view: nothing to carry over
    counts = [x.s.get_counts(v) for v in range(c.M)]
    members = [load(c, 0, cut, counts), load(c, cut, c.D, counts)]
    try:
        g = NativeGroup.__new__(NativeGroup)                                 # (no collective is needed for this: the local members)
        g.members, g.g = members, None
        items, weights = ec.queries(c, 30)
        for n in (1, 20, c.D + 3):
            one = x.s.predict_entities(c.m, x.weights, n, items=items, weights=weights)
            two = g.predict_entities(c.m, x.weights, n, items=items, weights=weights, **FORCED)
            assert one.ids.tobytes() == two.ids.tobytes() and one.scores.tobytes() == two.scores.tobytes() and one.counts.tobytes() == two.counts.tobytes()
            assert two.stats.cells == one.stats.cells and two.stats.excluded == one.stats.excluded
        psi = Ref(x, items, weights).psi
        one, two = x.s.predict_entities(c.m, x.weights, 20, psi=psi), g.predict_entities(c.m, x.weights, 20, psi=psi)
        assert one.ids.tobytes() == two.ids.tobytes() and one.scores.tobytes() == two.scores.tobytes()
    finally:
        for s in members:
            s.close()


def test_same_bytes_twice_knobs_change_nothing_and_nothing_of_the_handle_moves(loaded):
    x = loaded(100)
    s, c = x.s, x.c
    z = [s.get_assignments(v) for v in range(c.M)]
    trees, written, tuning = s.trees_current(), s.counts_written(), bytes(s.get_tuning())
    items, weights = ec.queries(c, 70)
    q, e = ec.pairs(c, 70, 0, c.D, 80, items, seed=1)
    kw = dict(items=items, weights=weights)
    one = s.predict_entities(c.m, x.weights, 20, **kw)
    p1 = s.rank_entities(c.m, x.weights, q, e, **kw)
    for knobs in ({}, FORCED, dict(block_entities=1), dict(block_queries=1), dict(block_entities=77, block_queries=3), dict(block_entities=10 ** 9, block_queries=10 ** 9)):
        two = s.predict_entities(c.m, x.weights, 20, **kw, **knobs)
        assert one.ids.tobytes() == two.ids.tobytes() and one.scores.tobytes() == two.scores.tobytes() and one.counts.tobytes() == two.counts.tobytes(), knobs
        assert two.stats.cells == one.stats.cells and two.stats.excluded == one.stats.excluded
        p2 = s.rank_entities(c.m, x.weights, q, e, **kw, **knobs)
        assert p1.score.tobytes() == p2.score.tobytes() and p1.rank.tobytes() == p2.rank.tobytes(), knobs
    nwk, nk = s.get_counts(c.m)
    assert np.array_equal(nwk, x.nwk) and np.array_equal(nk, x.nk) and all(np.array_equal(z[v], s.get_assignments(v)) for v in range(c.M))
    assert s.trees_current() == trees and s.counts_written() == written and bytes(s.get_tuning()) == tuning
    # a sub-range lists the same entities as the whole range cut to it
    part = s.predict_entities(c.m, x.weights, c.D, c0=40, c1=90, exclude_present=False, **kw)
    whole = s.predict_entities(c.m, x.weights, c.D, exclude_present=False, **kw)
    for j in range(70):
        keep = [i for i in range(whole.counts[j]) if 40 <= whole.ids[j, i] < 90]
        assert part.counts[j] == 50 and part.ids[j, :50].tolist() == whole.ids[j, keep].tolist()
        assert np.array_equal(bits(part.scores[j, :50]), bits(whole.scores[j, keep]))


def test_error_paths_leave_every_output_untouched(loaded):
    x = loaded(15)
    s, c = x.s, x.c
    D, K, V = c.D, c.K, c.V[c.m]
    w = np.ascontiguousarray(x.weights)
    off = np.array([0, 1, 3], dtype=np.int64)
    it = np.array([2, 0, 5], dtype=np.int32)
    keep = []

    def args(m=c.m, weights=w, c0=0, c1=D, nq=2, q_off=off, q_items=it, q_w=None, psi=None, be=0, bq=0):
        arrs = [None if a is None else np.ascontiguousarray(a) for a in (weights, q_off, q_items, q_w, psi)]
        keep.append(arrs)                                                    # the struct holds bare pointers
        p = [None if a is None else a.ctypes.data for a in arrs]
        return _lib.EntitiesArgsC(m, 1, p[0], c0, c1, nq, p[1], p[2], p[3], p[4], be, bq)

    def predict(a, n, code, null=None, h=None, nq=2):
        outs = [np.full((nq, 4), -7, dtype=np.int64), np.full((nq, 4), -7.0), np.full(nq, -7, dtype=np.int32)]
        st = _lib.EntitiesStatsC(-7, -7, -7, -7.0)
        ptr = [None if null == i else o.ctypes.data for i, o in enumerate(outs)]
        rc = s.L.mvhdp_predict_entities(h or s.h, None if a is None else C.byref(a), n, *ptr, C.byref(st))
        assert rc == code, (rc, code, s.L.mvhdp_last_error(s.h))
        assert all((o == -7).all() for o in outs)
        assert code == 0 or (st.cells, st.excluded, st.blocks, st.kernel_ms) == (-7, -7, -7, -7.0)
        return st

    def rank(a, query, entity, code, null=None):
        query, entity = np.array(query, dtype=np.int64), np.array(entity, dtype=np.int64)
        outs = [np.full(len(query) + 1, -7.0), np.full(len(query) + 1, -7, dtype=np.int64)]
        ptr = [None if null == i else o.ctypes.data for i, o in enumerate(outs)]
        rc = s.L.mvhdp_rank_entities(s.h, None if a is None else C.byref(a), len(query), query.ctypes.data, entity.ctypes.data, *ptr)
        assert rc == code, (rc, code, s.L.mvhdp_last_error(s.h))
        assert all((o == -7).all() for o in outs)

    predict(None, 4, INV); predict(args(m=3), 4, INV); predict(args(m=-1), 4, INV)
    predict(args(c0=-1), 4, INV); predict(args(c1=D + 1), 4, INV); predict(args(c0=5, c1=4), 4, INV)
    predict(args(nq=-1), 4, INV); predict(args(), 0, INV); predict(args(), -3, INV); predict(args(), 1025, INV)
    for i in range(3):
        predict(args(), 4, INV, null=i)
    predict(args(q_off=None), 4, INV); predict(args(q_items=None), 4, INV)
    predict(args(q_off=np.array([1, 1, 3], dtype=np.int64)), 4, INV)         # does not start at 0
    predict(args(q_off=np.array([0, 2, 1], dtype=np.int64)), 4, INV)         # decreases
    predict(args(q_items=np.array([2, V, 5], dtype=np.int32)), 4, INV)       # unlike a corpus token, an item >= V_m is an error
    predict(args(q_items=np.array([2, -1, 5], dtype=np.int32)), 4, INV)
    for bad in (-1.0, np.nan, np.inf, 2.0 ** 53 * 2):
        predict(args(q_w=np.array([1.0, bad, 1.0])), 4, INV)
    for bad in (-1e-300, np.nan, np.inf):
        psi = np.full((2, K), 0.25); psi[1, K - 1] = bad
        predict(args(psi=psi, q_off=None, q_items=None), 4, INV)
    predict(args(weights=None), 4, INV)
    for bad in ([1.0, -0.5, 1.0], [0.0, 0.0, 0.0], [1.0, np.nan, 0.0], [np.inf, 0.0, 0.0]):
        predict(args(weights=np.array(bad)), 4, INV)
    predict(args(be=-1), 4, INV); predict(args(bq=-1), 4, INV)
    st = predict(args(nq=0), 4, 0)                                           # no query: OK, only stats written
    assert (st.cells, st.excluded, st.blocks) == (0, 0, 0)
    rank(None, [0], [0], INV); rank(args(), [2], [0], INV); rank(args(), [-1], [0], INV); rank(args(), [0], [D], INV)
    rank(args(c0=3, c1=9), [0], [2], INV); rank(args(c0=3, c1=9), [0], [9], INV); rank(args(c0=4, c1=4), [0], [4], INV); rank(args(nq=0), [0], [0], INV)
    rank(args(), [0], [0], INV, null=0); rank(args(), [0], [0], INV, null=1); rank(args(m=7), [0], [0], INV)
    rank(args(q_w=np.array([1.0, -2.0, 1.0])), [0], [0], INV)
    rank(args(), [], [], 0); rank(args(c0=4, c1=4), [], [], 0)               # no pair: OK, nothing written
    with NativeSampler(c.K, c.V) as fresh:                                   # corpus and hyper-parameters, but no counts yet
        for v in range(c.M):
            fresh.set_corpus(v, c.doc_off[v], c.tokens[v])
        fresh.set_hyper(c.hy)
        predict(args(), 4, STATE, h=fresh.h)
    # an empty candidate range: every count 0, the slots unused
    got = s.predict_entities(c.m, x.weights, 4, items=[[2], [0, 5]], c0=9, c1=9)
    assert (got.counts == 0).all() and (got.ids == -1).all() and (got.scores == 0.0).all() and got.stats.cells == 0
    # a weight of exactly 2^53 and a psi of -0.0 are admitted
    s.predict_entities(c.m, x.weights, 4, items=[[2]], weights=[[2.0 ** 53]])
    z = np.zeros((1, K)); z[0, 0] = -0.0
    got = s.predict_entities(c.m, x.weights, 4, psi=z)
    assert got.ids[0].tolist() == [0, 1, 2, 3] and (bits(got.scores) == 0).all()
    Ref(x, [[2], [0, 5]]).check_predict(4, True, what="after the errors")   # and the handle still answers
