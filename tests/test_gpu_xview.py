"""mvhdp_predict_items / mvhdp_score_items on a device against the sequential restatement of their contract (tests/native/xview_ref.c):
items, counts and ranks equal, every score bit for bit.  theta is what mvhdp_doc_topic_proportions returns for the same handle (the
contract says so), phi and the chain are the restatement's own.  The comparison target is the restatement, never the device's output.
Shapes (tests/xview_cases.py): K below, at and above the 16-topic slab and ragged; types and entities below, at and above the 128 x 64
tile; a three-view model predicting view 1 from the others and a one-view model predicting itself; equal count rows (ties), an entity
that holds every type, one without the target view, one without any source view (the carry-over)."""
import ctypes as C

import numpy as np
import pytest

from mvtopicmodel_amd import MvhdpError, NativeSampler, _lib
from mvtopicmodel_amd.native import SWEEP_LIVE, SWEEP_NO_APPLY, NativeGroup
from tests import xview_cases as xc
from tests import xview_ref as xr
from tests.helpers import INV, STATE, load

pytestmark = pytest.mark.gpu


class Loaded:
    """the case in a sampler, and the restatement's scores [D][V_m] of the sampler's own theta and counts (computed once)"""

    def __init__(self, c, s=None):
        self.c, self.s = c, s or load(c)
        self.refresh()

    def refresh(self):
        c, s = self.c, self.s
        self.nwk, self.nk = s.get_counts(c.m)
        self.theta = s.doc_topic_proportions(c.weights)
        self.phi = xr.phi_table(self.nwk, self.nk, c.hy.beta[c.m], c.hy.beta_sum[c.m], c.hy.inactive)
        self.S = xr.scores(self.theta, self.phi)
        self.off, self.tok = c.doc_off[c.m], c.tokens[c.m]

    def pairs(self, n, seed=0):
        """unsorted, with repeats; a share of them items the entity holds itself"""
        rng = np.random.default_rng(seed)
        ent = rng.integers(0, self.c.D, n).astype(np.int64)
        item = rng.integers(0, self.c.V[self.c.m], n).astype(np.int32)
        for i in range(0, n, 3):
            b, e = self.off[ent[i]], self.off[ent[i] + 1]
            if e > b:
                item[i] = self.tok[rng.integers(b, e)]
        ent[n // 2:n // 2 + 2] = ent[0]; item[n // 2:n // 2 + 2] = item[0]  # the same pair three times
        return ent, item

    def check_predict(self, n, excl=True, S=None, theta=None, d0=0, d1=None, what=""):
        c = self.c
        d1 = c.D if d1 is None else d1
        S = self.S if S is None else S
        off = self.off[d0:d1 + 1] - self.off[d0]
        want = xr.predict(S[d0:d1], n, excl, off, self.tok[self.off[d0]:self.off[d1]])
        got = self.s.predict_items(c.m, None if theta is not None else c.weights, n, d0, d1, excl, theta)
        assert np.array_equal(got[2], want[2]), (what, n, np.flatnonzero(got[2] != want[2])[:8])
        assert np.array_equal(got[0], want[0]), (what, n, np.argwhere(got[0] != want[0])[:8])
        assert got[1].dtype == np.float64 and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64)), (what, n)
        return got

    def check_pairs(self, ent, item, excl=True, S=None, theta=None, what=""):
        c = self.c
        S = self.S if S is None else S
        want = xr.score_pairs(S, ent, item, excl, self.off, self.tok)
        got = self.s.score_items(c.m, None if theta is not None else c.weights, ent, item, 0, None, excl, theta)
        assert np.array_equal(got.score.view(np.uint64), want[0].view(np.uint64)), (what, np.flatnonzero(got.score != want[0])[:8])
        assert np.array_equal(got.rank, want[1]), (what, np.flatnonzero(got.rank != want[1])[:8])
        return got


@pytest.fixture(scope="module")
def loaded():
    made = {}

    def get(shape):
        if shape not in made:
            made[shape] = Loaded(xc.make(*shape))
        return made[shape]
    yield get
    for x in made.values():
        x.s.close()


@pytest.mark.parametrize("shape", xc.SHAPES, ids=str)
def test_shapes_equal_the_restatement(loaded, shape):
    x = loaded(shape)
    c = x.c
    V = c.V[c.m]
    nwk, nk = c.counts(c.m)
    assert np.array_equal(nwk, x.nwk) and np.array_equal(nk, x.nk)           # the sampler counted what the case holds
    if V >= 3 and c.D > 1:
        assert np.array_equal(nwk[V - 1], nwk[V - 2]) and (x.S[:, V - 1] == x.S[:, V - 2]).all()   # equal rows: the id decides
    for n in sorted({1, 20, V, V + 5}):
        items, scores, counts = x.check_predict(n, True, what=shape)
        if c.full >= 0:
            assert counts[c.full] == 0 and (items[c.full] == -1).all() and (scores[c.full] == 0.0).all()
        if c.no_target >= 0:
            assert counts[c.no_target] == min(n, V)
    x.check_predict(20, False, what=shape)
    ent, item = x.pairs(90, seed=shape[0])
    if c.full >= 0:
        ent[1], item[1] = c.full, V - 1                                      # a queried item of the entity that holds every type
    got = x.check_pairs(ent, item, True, what=shape)
    x.check_pairs(ent, item, False, what=shape)
    if c.full >= 0:
        assert got.rank[1] == 0                                              # nothing else is left to precede it
    if c.no_source >= 0:                                                     # carried over: the proportions of the entity in front of it
        d = c.no_source
        assert np.array_equal(x.theta[d], x.theta[d - 1]) and (x.theta[d] > 0).all()
    assert 0.0 <= got.recall_at(10) <= 1.0 and 0.0 < got.mrr() <= 1.0 and got.mean_log_score() < 0.0
    assert got.mrr() == float(np.mean(1.0 / (got.rank + 1.0))) and got.recall_at(10) == float(np.mean(got.rank < 10))


@pytest.mark.parametrize("V", [8192, 8193])
def test_the_selection_on_both_sides_of_its_lds_threshold(V):
    """a row of keys of up to 64 KiB (8192 types) is selected from LDS, a longer one from the block of scores itself; few tokens for so
    many types: nearly every count row is empty, so nearly every score is tied and the type id decides"""
    x = Loaded(xc.make(5, V, 3, 1))
    try:
        for n in (1, 20, V + 5):
            x.check_predict(n, True, what=V)
        x.check_predict(20, False, what=V)
        ent, item = x.pairs(30, seed=V)
        x.check_pairs(ent, item, True, what=V)
    finally:
        x.s.close()


def test_two_calls_same_bits_and_nothing_of_the_handle_moves(loaded):
    x = loaded((100, 128, 65, 3))
    s, c = x.s, x.c
    z = [s.get_assignments(v) for v in range(c.M)]
    trees, tuning = s.trees_current(), bytes(s.get_tuning())
    ent, item = x.pairs(60, seed=1)
    one, two = s.predict_items(c.m, c.weights, 20), s.predict_items(c.m, c.weights, 20)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, two))
    p1, p2 = s.score_items(c.m, c.weights, ent, item), s.score_items(c.m, c.weights, ent, item)
    assert p1.score.tobytes() == p2.score.tobytes() and p1.rank.tobytes() == p2.rank.tobytes()
    nwk, nk = s.get_counts(c.m)
    assert np.array_equal(nwk, x.nwk) and np.array_equal(nk, x.nk) and all(np.array_equal(z[v], s.get_assignments(v)) for v in range(c.M))
    assert s.trees_current() == trees and bytes(s.get_tuning()) == tuning
    # a sub-range is the same rows
    part = x.check_predict(20, True, d0=7, d1=40, what="range")
    assert part[0].tobytes() == one[0][7:40].tobytes() and part[1].tobytes() == one[1][7:40].tobytes()


def test_borders_between_blocks_stripes_and_ranges(loaded, monkeypatch):
    """8 KiB instead of 256 MiB: K = 100 -> theta ranges of 10 entities and phi stripes of 10 types, V = 128 -> score blocks of 8 rows"""
    x = loaded((100, 128, 65, 3))
    monkeypatch.setenv("MVHDP_XVIEW_BLOCK_BYTES", "8192")
    x.check_predict(20, True, what="borders")
    x.check_predict(133, False, what="borders")
    ent, item = x.pairs(120, seed=2)
    x.check_pairs(ent, item, True, what="borders")
    x.check_pairs(ent[:1], item[:1], False, what="borders, one pair")


def test_inactive_topics_are_exact_zeros():
    inactive = np.zeros(64, dtype=np.uint8)
    inactive[[0, 17, 63]] = 1
    x = Loaded(xc.make(64, 127, 65, 3, inactive=inactive))
    try:
        assert (x.phi[:, [0, 17, 63]] == 0.0).all() and (x.phi[:, 1] > 0.0).all()
        x.check_predict(20, True, what="inactive")
        x.check_pairs(*x.pairs(60), True, what="inactive")
        plain = xr.scores(x.theta, xr.phi_table(x.nwk, x.nk, x.c.hy.beta[1], x.c.hy.beta_sum[1]))
        assert (plain != x.S).mean() > 0.5                                   # ... and that is seen in the scores
    finally:
        x.s.close()


def test_after_a_live_sweep_and_behind_a_no_apply_sweep():
    x = Loaded(xc.make(64, 127, 65, 3, seed=1))
    s, c = x.s, x.c
    try:
        before = x.S.copy()
        s.sweep(0, 11, flags=SWEEP_LIVE)
        x.refresh()
        assert (x.S != before).any()
        x.check_predict(20, True, what="live")
        x.check_pairs(*x.pairs(60), True, what="live")
        s.sweep(1, 11, flags=SWEEP_NO_APPLY)                                 # its deltas wait: the counts are not the model's
        for call in (lambda: s.predict_items(c.m, c.weights, 5), lambda: s.score_items(c.m, c.weights, [0], [0]),
                     lambda: s.predict_items(c.m, None, 5, theta=x.theta)):
            with pytest.raises(MvhdpError) as e:
                call()
            assert e.value.code == STATE and "pending" in str(e.value)
        s.apply_delta()
        x.refresh()
        x.check_predict(20, True, what="applied")
        s.set_assignments(0, s.get_assignments(0))                           # assignments replaced: the counts are stale until recounted
        with pytest.raises(MvhdpError) as e:
            s.predict_items(c.m, c.weights, 5)
        assert e.value.code == STATE
        s.build_counts()
        x.check_predict(20, True, what="recounted")
    finally:
        s.close()


def test_a_theta_override_that_puts_two_types_one_ulp_apart(loaded):
    x = loaded((64, 127, 300, 3))
    c = x.c
    K, V = c.K, c.V[c.m]
    # types a, b: equal phi at topic k0 (no count of either), different at k1; theta = e_k0 + t e_k1: score = fma(t, phi[.][k1], phi[.][k0]),
    # and t is searched, with the restatement, until the two scores are neighbours
    found = None
    for a in range(V - 2):
        for b in range(a + 1, V - 2):
            k1 = np.flatnonzero(x.nwk[a] != x.nwk[b])
            k0 = np.flatnonzero((x.nwk[a] == 0) & (x.nwk[b] == 0))
            if len(k1) == 0 or len(k0) == 0:
                continue
            k0, k1 = int(k0[0]), int(k1[0])
            base, gap = x.phi[a, k0], abs(x.phi[a, k1] - x.phi[b, k1])
            for f in np.linspace(0.6, 1.4, 33):
                t = float(np.spacing(base) / gap * f)
                row = np.zeros(K); row[k0] = 1.0; row[k1] = t
                sa, sb = xr.chain(row, x.phi[a]), xr.chain(row, x.phi[b])
                if sa != sb and (np.nextafter(sa, sb) == sb):
                    found = (a, b, row)
                    break
            if found:
                break
        if found:
            break
    assert found, "no pair of types one ulp apart"
    a, b, row = found
    theta = np.tile(row, (c.D, 1))
    theta[1::2] = x.theta[1::2]                                              # every other entity keeps its own proportions
    S = xr.scores(theta, x.phi)
    assert abs(int(S[0, a:a + 1].view(np.int64)[0]) - int(S[0, b:b + 1].view(np.int64)[0])) == 1
    x.check_predict(V, False, S=S, theta=theta, what="ulp")
    x.check_predict(20, True, S=S, theta=theta, what="ulp")
    ent = np.array([0, 0, 2, 2, 1], dtype=np.int64)
    got = x.check_pairs(ent, np.array([a, b, b, a, a], dtype=np.int32), False, S=S, theta=theta, what="ulp")
    assert abs(int(got.rank[0]) - int(got.rank[1])) >= 1 and got.score[0] != got.score[1]
    with pytest.raises(MvhdpError) as e:                                     # the override is checked: finite and >= 0
        bad = theta.copy(); bad[3, 5] = -1e-300
        x.s.predict_items(c.m, None, 5, theta=bad)
    assert e.value.code == INV
    with pytest.raises(MvhdpError) as e:
        bad = theta.copy(); bad[c.D - 1, K - 1] = np.inf
        x.s.score_items(c.m, c.weights, [0], [0], theta=bad)
    assert e.value.code == INV


def test_rows_whose_scores_are_all_equal_are_listed_by_type_alone(loaded):
    """a theta row of zeros: every score of the row is +0.0, every key equal, and the selection has no bit to descend on; what is
    listed is the first types that are not excluded, in ascending id"""
    x = loaded((100, 128, 65, 3))
    c = x.c
    V = c.V[c.m]
    holder = next(d for d in range(c.D) if d != c.full and x.off[d + 1] - x.off[d] >= 2)
    rows = [holder, c.full]                                                  # one holds a few types, one every type
    theta = x.theta.copy()
    theta[rows] = 0.0
    S = xr.scores(theta, x.phi)
    assert (S[rows].view(np.uint64) == 0).all() and (np.delete(S, rows, axis=0) > 0.0).all()
    for n in (5, V + 5):
        for excl in (True, False):
            items, scores, counts = x.check_predict(n, excl, S=S, theta=theta, what=("equal", n, excl))
            for d in rows:
                held = set(x.tok[x.off[d]:x.off[d + 1]].tolist()) if excl else set()
                first = [w for w in range(V) if w not in held][:n]
                assert counts[d] == len(first) and items[d, :len(first)].tolist() == first and (items[d, len(first):] == -1).all()
                assert (scores[d].view(np.uint64) == 0).all()
            assert counts[c.full] == (0 if excl else min(n, V)) and 0 < counts[holder] <= min(n, V)


def test_error_paths_leave_every_output_untouched(loaded):
    x = loaded((5, 3, 65, 3))
    s, c = x.s, x.c
    D, w = c.D, np.ascontiguousarray(c.weights)

    keep = []

    def args(m=c.m, weights=w, theta=None):
        keep.append((weights, theta))                                        # the struct holds bare pointers
        return _lib.PredictArgsC(m, 1, None if weights is None else weights.ctypes.data, None if theta is None else theta.ctypes.data)

    def predict(a, d0, d1, n, code, null=None, h=None):
        outs = [np.full((D, 4), -7, dtype=np.int32), np.full((D, 4), -7.0), np.full(D, -7, dtype=np.int32)]
        ptr = [None if null == i else o.ctypes.data for i, o in enumerate(outs)]
        rc = s.L.mvhdp_predict_items(h or s.h, None if a is None else C.byref(a), d0, d1, n, *ptr)
        assert rc == code, (rc, code, s.L.mvhdp_last_error(s.h))
        assert all((o == -7).all() for o in outs)

    def score(a, d0, d1, ent, item, code):
        ent, item = np.array(ent, dtype=np.int64), np.array(item, dtype=np.int32)
        outs = [np.full(len(ent) + 1, -7.0), np.full(len(ent) + 1, -7, dtype=np.int32)]
        rc = s.L.mvhdp_score_items(s.h, C.byref(a), d0, d1, len(ent), ent.ctypes.data, item.ctypes.data, outs[0].ctypes.data, outs[1].ctypes.data)
        assert rc == code, (rc, code, s.L.mvhdp_last_error(s.h))
        assert all((o == -7).all() for o in outs)

    predict(args(m=3), 0, D, 4, INV); predict(args(m=-1), 0, D, 4, INV); predict(None, 0, D, 4, INV)
    predict(args(), -1, D, 4, INV); predict(args(), 0, D + 1, 4, INV); predict(args(), 5, 4, 4, INV)
    predict(args(), 0, D, 0, INV); predict(args(), 0, D, -3, INV)
    for i in range(3):
        predict(args(), 0, D, 4, INV, null=i)
    predict(args(weights=None), 0, D, 4, INV)                                # neither weights nor theta
    for bad in ([1.0, -0.5, 1.0], [0.0, 0.0, 0.0], [1.0, np.nan, 0.0], [np.inf, 0.0, 0.0]):
        predict(args(weights=np.array(bad)), 0, D, 4, INV)
    predict(args(), 9, 9, 4, 0)                                              # an empty range: OK, nothing written
    score(args(), 0, D, [0, D], [0, 0], INV); score(args(), 3, 9, [2], [0], INV); score(args(), 0, D, [0], [3], INV); score(args(), 0, D, [0], [-1], INV)
    score(args(m=7), 0, D, [0], [0], INV)
    score(args(), 0, D, [], [], 0); score(args(), 4, 4, [], [], 0)
    with NativeSampler(c.K, c.V) as fresh:                                   # corpus and hyper-parameters, but no counts yet
        for v in range(c.M):
            fresh.set_corpus(v, c.doc_off[v], c.tokens[v])
        fresh.set_hyper(c.hy)
        predict(args(), 0, D, 4, STATE, h=fresh.h)
    with pytest.raises(MvhdpError) as e:
        s.predict_items(c.m, c.weights, 0)
    assert e.value.code == INV and "n < 1" in str(e.value)
    x.check_predict(4, True, what="after the errors")                        # and the handle still answers


def test_a_group_of_two_members_equals_one_handle(loaded):
    x = loaded((100, 128, 65, 3))
    c = x.c
    lens = [np.diff(c.doc_off[v]) for v in range(c.M)]
    cut = next(d for d in range(c.D // 2, c.D) if all(l[d] > 0 for l in lens))   # the second member's first entity has every view: nothing to carry over
    counts = [x.s.get_counts(v) for v in range(c.M)]
    members = [load(c, 0, cut, counts), load(c, cut, c.D, counts)]
    try:
        g = NativeGroup.__new__(NativeGroup)                                 # (no collective is needed for this: the local members, as topic_phrases)
        g.members, g.g = members, None
        one = x.s.predict_items(c.m, c.weights, 20)
        two = g.predict_items(c.m, c.weights, 20)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one, two))
        part = g.predict_items(c.m, c.weights, 7, cut - 5, cut + 9, exclude_present=False)
        want = x.s.predict_items(c.m, c.weights, 7, cut - 5, cut + 9, exclude_present=False)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(part, want))
        ent, item = x.pairs(80, seed=5)
        p1, p2 = x.s.score_items(c.m, c.weights, ent, item), g.score_items(c.m, c.weights, ent, item)
        assert p1.score.tobytes() == p2.score.tobytes() and p1.rank.tobytes() == p2.rank.tobytes()
        t1 = g.predict_items(c.m, None, 20, theta=x.theta)                   # an override is cut along with the entities
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one, t1))
    finally:
        for s in members:
            s.close()
