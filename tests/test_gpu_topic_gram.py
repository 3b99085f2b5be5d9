"""mvhdp_topic_gram on a device against the sequential restatement of its contract (tests/native/gram_ref.c): every fp64 bit pattern of
gram and sums, every integer of n_above and co_above.  phi is xview_ref's, theta is what mvhdp_doc_topic_proportions returns for the same
handle (the contract says so); the blocks, the chains, the order of the blocks and the counts are the restatement's own.  The comparison
target is the restatement, never the device's output.  Shapes (tests/gram_cases.py): K below, at and above the 64 x 128 tile and the
64-topic mask tile; rows below, at and above the 16-row slab, the 64-row mask word and the 1024-row block; one, two and all blocks per
pass.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from mvtopicmodel_amd import MvhdpError, NativeSampler, _lib
from mvtopicmodel_amd.native import SWEEP_LIVE, SWEEP_NO_APPLY, NativeGroup, merge_topic_grams
from tests import gram_cases as gc
from tests import gram_ref as gr
from tests import xview_ref as xr
from tests.helpers import INV, STATE, bits, load

pytestmark = pytest.mark.gpu


def check(got, x, transform="identity", threshold=None, what=""):
    """got: the device's TopicGram; x: the rows it stands for"""
    want = gr.topic_gram(x, transform, threshold)
    assert got.gram.dtype == np.float64 and got.sums.dtype == np.float64
    assert np.array_equal(bits(got.gram), bits(want.gram)), (what, np.argwhere(bits(got.gram) != bits(want.gram))[:8])
    assert np.array_equal(bits(got.sums), bits(want.sums)), (what, np.flatnonzero(bits(got.sums) != bits(want.sums))[:8])
    assert np.array_equal(bits(got.gram), bits(got.gram.T)), what
    if threshold is None:
        assert got.n_above is None and got.co_above is None
    else:
        assert got.n_above.dtype == np.int64 and got.co_above.dtype == np.int64
        assert np.array_equal(got.n_above, want.n_above), (what, np.flatnonzero(got.n_above != want.n_above)[:8])
        assert np.array_equal(got.co_above, want.co_above), (what, np.argwhere(got.co_above != want.co_above)[:8])
        assert np.array_equal(np.diag(got.co_above), got.n_above)
    blocks = (len(x) + gr.BLOCK_ROWS - 1) // gr.BLOCK_ROWS
    assert got.rows == len(x) and got.stats.rows == len(x) and got.stats.blocks == blocks and got.transform == transform
    return want


@pytest.fixture(scope="module")
def bare():
    """samplers that supply only the device, the stream and K"""
    made = {}

    def get(K):
        if K not in made:
            made[K] = NativeSampler(K, [3])
        return made[K]
    yield get
    for s in made.values():
        s.close()


@pytest.mark.parametrize("K", gc.K_VALUES)
def test_host_rows_of_every_shape_equal_the_restatement(bare, K):
    s = bare(K)
    for n in gc.ROW_VALUES:
        x = gc.rows(n, K)
        blocks = (n + 1023) // 1024
        for transform in ("identity", "sqrt"):
            want = gr.topic_gram(x, transform, gc.THRESHOLD)
            for bpp in gc.BLOCKS_PER_PASS:
                got = s.topic_gram(x, transform=transform, threshold=gc.THRESHOLD, blocks_per_pass=bpp)
                what = (K, n, transform, bpp)
                assert np.array_equal(bits(got.gram), bits(want.gram)), (what, np.argwhere(bits(got.gram) != bits(want.gram))[:8])
                assert np.array_equal(bits(got.sums), bits(want.sums)), what
                assert np.array_equal(bits(got.gram), bits(got.gram.T)), what
                assert np.array_equal(got.n_above, want.n_above) and np.array_equal(got.co_above, want.co_above), what
                assert (got.stats.rows, got.stats.blocks) == (n, blocks) and got.rows == n
                assert got.stats.passes == (blocks if bpp == 1 else (blocks + 1) // 2 if bpp == 2 else min(blocks, 1)), what
    if K == 17:
        x = gc.rows(3 * 1024 + 5, K)
        assert s.topic_gram(x, blocks_per_pass=1).stats.passes == 4          # at least three passes happened
        check(s.topic_gram(x, r0=1000, r1=2100, threshold=gc.THRESHOLD), x[1000:2100], "identity", gc.THRESHOLD, "a cut of the host rows")
        check(s.topic_gram(x), x, what="no threshold: no counts")


def test_host_values_zeros_overflow_subnormal_and_wide_magnitudes(bare):
    K = 17
    s = bare(K)
    x = gc.rows(1500, K, seed=7)
    x[:, 3] = 0.0                                                            # whole zero columns, and a zero row
    x[:, 16] = 0.0
    x[700] = 0.0
    want = check(s.topic_gram(x, threshold=0.0), x, "identity", 0.0, "zeros")
    assert not bits(want.gram[3]).any() and not bits(want.sums[[3, 16]]).any() and want.n_above[3] == 0      # +0.0, never -0.0
    check(s.topic_gram(np.zeros((1030, K)), transform="sqrt", threshold=0.0), np.zeros((1030, K)), "sqrt", 0.0, "all zero")
    # a cell that overflows to +inf, and one that lands subnormal
    x = gc.rows(1100, K, seed=8)
    x[:, 0] = 1e200
    x[5, 1] = 1e120
    x[:, 2] = 0.0
    x[9, 2] = 2.0 ** -530
    want = check(s.topic_gram(x, blocks_per_pass=1), x, what="overflow and subnormal")
    assert want.gram[0, 0] == np.inf and want.gram[0, 1] == np.inf and np.isfinite(want.gram[1, 1]) and np.isfinite(want.sums).all()
    assert 0.0 < want.gram[2, 2] < np.finfo(np.float64).tiny and want.gram[2, 2] == 2.0 ** -1060
    # magnitudes from 2^-300 to 2^300 under the sqrt
    x = gc.wide_rows(2100, K)
    assert x.min() < 2.0 ** -290 and x.max() > 2.0 ** 290
    want = check(s.topic_gram(x, transform="sqrt", threshold=1.0), x, "sqrt", 1.0, "wide")
    assert np.isfinite(want.gram).all()
    sub = np.full((70, K), 5e-324)                                           # subnormal entries: their roots are normal numbers
    sub[::3] = 2.0 ** -1040
    check(s.topic_gram(sub, transform="sqrt"), sub, "sqrt", None, "subnormal entries")


def test_the_threshold_is_strict_and_infinite_thresholds(bare):
    K = 65
    s = bare(K)
    x = gc.rows(1100, K, seed=9)
    at, above = gc.THRESHOLD, np.nextafter(gc.THRESHOLD, 1.0)
    assert (x == at).sum() > 100 and (x == above).sum() > 100
    want = check(s.topic_gram(x, threshold=at), x, "identity", at, "at the threshold")
    assert np.array_equal(want.n_above, (x >= above).sum(0)) and (want.n_above < (x >= at).sum(0)).all()
    up = check(s.topic_gram(x, threshold=above), x, "identity", above, "one ulp above")
    assert np.array_equal(want.n_above - up.n_above, (x == above).sum(0))
    every = check(s.topic_gram(x, threshold=-np.inf, transform="sqrt"), x, "sqrt", -np.inf, "-inf")
    assert (every.n_above == 1100).all() and (every.co_above == 1100).all()
    none = check(s.topic_gram(x, threshold=np.inf), x, "identity", np.inf, "+inf")
    assert not none.n_above.any() and not none.co_above.any()
    # either integer output alone
    a = _lib.TopicGramArgsC(2, 0, 0, 0, None, x.ctypes.data, 0, len(x), at)
    for only in (0, 1):
        gram, sums = np.zeros((K, K)), np.zeros(K)
        na, co = np.zeros(K, dtype=np.int64), np.zeros((K, K), dtype=np.int64)
        assert s.L.mvhdp_topic_gram(s.h, C.byref(a), gram.ctypes.data, sums.ctypes.data, na.ctypes.data if only == 0 else None, co.ctypes.data if only == 1 else None, None) == 0
        assert np.array_equal(bits(gram), bits(want.gram)) and np.array_equal(bits(sums), bits(want.sums))
        assert np.array_equal(na, want.n_above) if only == 0 else np.array_equal(co, want.co_above)


@pytest.fixture(scope="module")
def words():
    """a three-view model whose view 1 has 2500 types (three blocks), with inactive topics"""
    inactive = np.zeros(65, dtype=np.uint8)
    inactive[[0, 17, 64]] = 1
    c = gc.model(65, 2500, 300, inactive=inactive)
    s = load(c)
    yield c, s
    s.close()


def phi_of(c, s, m):
    nwk, nk = s.get_counts(m)
    return xr.phi_table(nwk, nk, c.hy.beta[m], c.hy.beta_sum[m], c.hy.inactive)


def test_words_after_build_counts_with_inactive_topics_and_a_sub_range(words):
    c, s = words
    for m in range(c.M):
        phi = phi_of(c, s, m)
        assert (phi[:, [0, 17, 64]] == 0.0).all() and (phi[:, 1] > 0.0).all()
        for transform in ("identity", "sqrt"):
            want = check(s.topic_gram("words", m=m, transform=transform, threshold=1e-3), phi, transform, 1e-3, ("words", m, transform))
            assert not bits(want.gram[17]).any() and want.n_above[17] == 0
    phi = phi_of(c, s, 1)
    for r0, r1, bpp in ((37, 2300, 0), (37, 2300, 1), (1025, 1026, 0), (2499, 2500, 0), (1, 1025, 2)):
        got = s.topic_gram("words", m=1, r0=r0, r1=r1, transform="sqrt", threshold=1e-3, blocks_per_pass=bpp)
        check(got, phi[r0:r1], "sqrt", 1e-3, ("words", r0, r1, bpp))
    bc = s.topic_gram("words", m=1, transform="sqrt").bhattacharyya()
    active = np.flatnonzero(c.hy.inactive == 0)
    assert np.allclose(np.diag(bc)[active], 1.0) and (bc[np.ix_(active, active)] <= 1.0 + 1e-12).all()


def test_entities_with_missing_views_across_r0_and_a_block_border():
    c = gc.model(17, 40, 2500, seed=3)
    s = load(c)
    try:
        w = c.weights                                                        # [1.0, 0.0, 0.7]: a zero among them
        assert (w == 0.0).any()
        theta = s.doc_topic_proportions(w)
        lacks = gc.lacks_a_weighted_view(c, w)
        r0 = next(d for d in range(1, c.D - 1024) if lacks[d] and lacks[d + 1024])      # the carry-over crosses r0 and the first block border
        assert lacks.sum() > 100
        for transform in ("identity", "sqrt"):
            check(s.topic_gram("entities", view_weights=w, transform=transform, threshold=0.05), theta, transform, 0.05, ("entities", transform))
        for a, b, bpp in ((r0, c.D, 0), (r0, c.D, 1), (r0, r0 + 1025, 0), (c.D - 1, c.D, 0)):
            check(s.topic_gram("entities", view_weights=w, r0=a, r1=b, threshold=0.05, blocks_per_pass=bpp), theta[a:b], "identity", 0.05, ("entities", a, b, bpp))
        w2 = np.array([0.0, 2.0, 0.5])
        theta2 = s.doc_topic_proportions(w2)
        assert (theta2 != theta).any()
        check(s.topic_gram("entities", view_weights=w2), theta2, what="other weights")
        corr = s.topic_gram("entities", view_weights=w).correlation()
        assert np.allclose(corr, np.corrcoef(theta.T), atol=1e-9)
        # after a live sweep: other assignments, other proportions, other counts
        s.sweep(0, 11, flags=SWEEP_LIVE)
        after = s.doc_topic_proportions(w)
        assert (after != theta).any()
        check(s.topic_gram("entities", view_weights=w, threshold=0.05), after, "identity", 0.05, "entities after a live sweep")
        check(s.topic_gram("words", m=0, transform="sqrt"), phi_of(c, s, 0), "sqrt", None, "words after a live sweep")
    finally:
        s.close()


def test_words_need_current_counts():
    c = gc.model(16, 70, 80, seed=1)
    with NativeSampler(c.K, c.V) as fresh:                                   # corpus and hyper-parameters, but no counts yet
        for v in range(c.M):
            fresh.set_corpus(v, c.doc_off[v], c.tokens[v])
            fresh.set_assignments(v, c.z[v])
        fresh.set_hyper(c.hy)
        with pytest.raises(MvhdpError) as e:
            fresh.topic_gram("words", m=1)
        assert e.value.code == STATE
        fresh.topic_gram("entities", view_weights=c.weights)                 # the proportions need no counts
    s = load(c)
    try:
        check(s.topic_gram("words", m=1), phi_of(c, s, 1), what="current")
        s.sweep(0, 11, flags=SWEEP_NO_APPLY)                                 # its deltas wait: the counts are not the model's
        with pytest.raises(MvhdpError) as e:
            s.topic_gram("words", m=1)
        assert e.value.code == STATE and "pending" in str(e.value)
        s.apply_delta()
        check(s.topic_gram("words", m=1), phi_of(c, s, 1), what="applied")
        s.set_assignments(0, s.get_assignments(0))                           # assignments replaced: the counts are stale until recounted
        with pytest.raises(MvhdpError) as e:
            s.topic_gram("words", m=1)
        assert e.value.code == STATE
        x = gc.rows(10, c.K)
        check(s.topic_gram(x), x, what="host rows need no counts")
        s.build_counts()
        check(s.topic_gram("words", m=1), phi_of(c, s, 1), what="recounted")
    finally:
        s.close()


def test_error_paths_leave_every_output_untouched(words):
    c, s = words
    K, D, V = c.K, c.D, c.V[1]
    w = np.ascontiguousarray(c.weights)
    x = gc.rows(5, K)
    keep = []

    def args(source=0, m=1, transform=0, bpp=0, weights=w, rows=x, r0=0, r1=5, thr=0.5):
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (weights, rows)]
        keep.append(arrs)                                                    # the struct holds bare pointers
        p = [None if a is None else a.ctypes.data for a in arrs]
        return _lib.TopicGramArgsC(source, m, transform, bpp, p[0], p[1], r0, r1, thr)

    def call(a, code, null=None, h=None):
        outs = [np.full((K, K), -7.0), np.full(K, -7.0), np.full(K, -7, dtype=np.int64), np.full((K, K), -7, dtype=np.int64)]
        st = _lib.TopicGramStatsC(-7, -7, -7, -7.0)
        ptr = [None if null == i else o.ctypes.data for i, o in enumerate(outs)]
        rc = s.L.mvhdp_topic_gram(h or s.h, None if a is None else C.byref(a), *ptr, C.byref(st))
        assert rc == code, (rc, code, s.L.mvhdp_last_error(s.h))
        if code != 0:
            assert all((o == -7).all() for o in outs) and (st.rows, st.blocks, st.passes, st.kernel_ms) == (-7, -7, -7, -7.0)
        return outs, st

    call(None, INV); call(args(), INV, null=0); call(args(), INV, null=1)
    call(args(source=3), INV); call(args(source=-1), INV); call(args(transform=2), INV); call(args(transform=-1), INV)
    call(args(bpp=-1), INV); call(args(thr=np.nan), INV)
    call(args(source=1, m=3), INV); call(args(source=1, m=-1), INV)
    for source, top in ((0, D), (1, V)):
        call(args(source=source, r0=-1), INV); call(args(source=source, r1=top + 1), INV); call(args(source=source, r0=5, r1=4), INV)
    call(args(source=2, r0=-1), INV); call(args(source=2, r0=5, r1=4), INV)
    call(args(weights=None), INV)
    for bad in ([1.0, -0.5, 1.0], [0.0, 0.0, 0.0], [1.0, np.nan, 0.0], [np.inf, 0.0, 0.0]):
        call(args(weights=np.array(bad)), INV)
    call(args(source=2, rows=None), INV)
    for bad in (-1e-300, np.nan, np.inf, -np.inf):
        y = x.copy(); y[4, K - 1] = bad
        call(args(source=2, rows=y), INV)
    # an empty range: OK, every output zero, no block
    for source in (0, 1, 2):
        outs, st = call(args(source=source, r0=3, r1=3), 0)
        assert all(not o.view(np.uint64).any() for o in outs) and (st.rows, st.blocks, st.passes) == (0, 0, 0)
    # a valid call writes everything, NULL integer outputs and NULL stats are allowed
    outs, st = call(args(source=2), 0)
    want = gr.topic_gram(x, "identity", 0.5)
    assert np.array_equal(bits(outs[0]), bits(want.gram)) and np.array_equal(outs[3], want.co_above) and (st.rows, st.blocks, st.passes) == (5, 1, 1)
    outs, _ = call(args(source=2), 0, null=2)
    assert (outs[2] == -7).all() and np.array_equal(outs[3], want.co_above)
    gram, sums = np.zeros((K, K)), np.zeros(K)
    a = args(source=2)
    assert s.L.mvhdp_topic_gram(s.h, C.byref(a), gram.ctypes.data, sums.ctypes.data, None, None, None) == 0
    assert np.array_equal(bits(gram), bits(want.gram))
    with pytest.raises(ValueError):
        s.topic_gram("topics")
    with pytest.raises(ValueError):
        s.topic_gram(x, transform="square")
    with pytest.raises(ValueError):
        s.topic_gram(np.zeros((4, K + 1)))


def test_same_bytes_twice_and_nothing_of_the_handle_moves(words):
    c, s = words
    z = [s.get_assignments(v) for v in range(c.M)]
    counts = [s.get_counts(v) for v in range(c.M)]
    trees, written, tuning = s.trees_current(), s.counts_written(), bytes(s.get_tuning())
    x = gc.rows(2100, c.K, seed=4)
    for kw in (dict(source="entities", view_weights=c.weights), dict(source="words", m=1, transform="sqrt"), dict(source=x, transform="sqrt")):
        one = s.topic_gram(threshold=0.01, **kw)
        for bpp in (0, 1, 2, 10 ** 6):
            two = s.topic_gram(threshold=0.01, blocks_per_pass=bpp, **kw)
            assert one.gram.tobytes() == two.gram.tobytes() and one.sums.tobytes() == two.sums.tobytes(), (kw.get("m"), bpp)
            assert one.n_above.tobytes() == two.n_above.tobytes() and one.co_above.tobytes() == two.co_above.tobytes(), (kw.get("m"), bpp)
    for v in range(c.M):
        nwk, nk = s.get_counts(v)
        assert np.array_equal(nwk, counts[v][0]) and np.array_equal(nk, counts[v][1]) and np.array_equal(z[v], s.get_assignments(v))
    assert s.trees_current() == trees and s.counts_written() == written and bytes(s.get_tuning()) == tuning


def test_a_group_of_two_members():
    c = gc.model(17, 40, 2300, seed=5)
    w = c.weights
    lens = [np.diff(c.doc_off[v]) for v in range(c.M)]
    cut = next(d for d in range(1100, c.D) if all(l[d] > 0 for l in lens))   # the second member's first entity has every view: nothing to carry over
    one = load(c)
    counts = [one.get_counts(v) for v in range(c.M)]
    members = [load(c, 0, cut, counts), load(c, cut, c.D, counts)]
    try:
        g = NativeGroup.__new__(NativeGroup)                                 # (no collective is needed for this: the local members)
        g.members, g.g = members, None
        for transform in ("identity", "sqrt"):
            single = one.topic_gram("entities", view_weights=w, transform=transform, threshold=0.05)
            both = g.topic_gram("entities", view_weights=w, transform=transform, threshold=0.05)
            assert np.array_equal(both.n_above, single.n_above) and np.array_equal(both.co_above, single.co_above) and both.rows == c.D
            shards = [gr.topic_gram(s.doc_topic_proportions(w), transform, 0.05) for s in members]
            want = merge_topic_grams(shards)
            assert np.array_equal(bits(both.gram), bits(want.gram)) and np.array_equal(bits(both.sums), bits(want.sums))
            assert np.array_equal(both.n_above, want.n_above) and np.array_equal(both.co_above, want.co_above)
            assert both.stats.blocks == sum((s.D + 1023) // 1024 for s in members)
        phi = phi_of(c, one, 1)
        check(g.topic_gram("words", m=1, transform="sqrt", threshold=1e-3), phi, "sqrt", 1e-3, "a group's words")
        x = gc.rows(100, c.K)
        check(g.topic_gram(x), x, what="a group's host rows")
    finally:
        for s in members + [one]:
            s.close()
