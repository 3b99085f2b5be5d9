"""mvhdp_fold_in on a device against the sequential restatement of its contract (tests/native/foldin_ref.c): z, counts_sum and the totals
as integers, theta bit for bit.  The comparison target is the restatement, never the device's own output -- except where the library's
other entry is the target: theta against mvhdp_doc_topic_proportions on a second handle that holds the returned z.
Shapes: K below, at and above the 64 lanes, ragged and several topics a lane (both gather paths); one and three views (the per-wave state
in LDS and in the global scratch); span lengths around the 64-lane width and of 0, 1, 2 tokens; views missing for some documents and for
all; out-of-vocabulary tokens first, in the middle, last; a document beyond the LDS cap of z; more documents than waves."""
import ctypes as C

import numpy as np
import pytest

from mvtopicmodel_amd import MvhdpError, NativeSampler, _lib, synth
from mvtopicmodel_amd.native import Hyper, NativeGroup
from tests import foldin_cases as fc
from tests import foldin_ref as fr
from tests.helpers import INV, STATE, uneven_hyper

pytestmark = pytest.mark.gpu
KS = [5, 64, 65, 100, 130, 1000]


def hyper(K, V, seed):
    """uneven_hyper with a zero in p_a: the default coupling has a zero entry"""
    hy = uneven_hyper(K, V, seed)
    if len(V) > 1:
        hy.p_a[0, len(V) - 1] = 0.0
        hy.p_a[1, 0] = 0.5
    return hy


class Model:
    """a sampler whose counts were reached by two deferred sweeps of a synthetic corpus, and the frozen model the restatement reads"""

    def __init__(self, K, V, seed=3, D=200):
        c = synth.generate(K, V, D, [40] + [6] * (len(V) - 1), seed=seed)
        rng = np.random.default_rng(seed)
        self.K, self.V, self.hy = K, V, hyper(K, V, seed)
        self.s = s = NativeSampler(K, V)
        for m in range(c.M):
            s.set_corpus(m, c.doc_off[m], c.tokens[m])
            s.set_assignments(m, rng.integers(0, K, len(c.tokens[m])).astype(np.int32))
        s.set_hyper(self.hy)
        s.build_counts()
        for it in range(2):
            s.sweep(it, 99)
        self.w = np.array([1.0] + [0.5, 0.25, 0.3, 0.2, 0.1, 0.7, 0.4][:len(V) - 1])

    def frozen(self):
        s, hy, M = self.s, self.hy, len(self.V)
        counts = [s.get_counts(m) for m in range(M)]
        alpha, inactive = s.get_alpha()
        return fr.Model([c[0] for c in counts], np.stack([c[1] for c in counts]), hy.beta, hy.beta_sum, hy.gamma, alpha[:, :self.K], hy.alpha_sum,
                        inactive, hy.p_a, hy.p_b)

    def close(self):
        self.s.close()


@pytest.fixture(scope="module")
def models():
    made = {}

    def get(K, M):
        if (K, M) not in made:
            V0 = 150 if K < 1000 else 200
            made[K, M] = Model(K, [V0, 30, 25, 20, 20, 20, 20, 20][:M], D=200 if M < 8 else 60)
        return made[K, M]
    yield get
    for mdl in made.values():
        mdl.close()


def assert_equals_ref(got, ref, what):
    assert (got.tokens, got.oov, got.visits) == (ref.tokens, ref.oov, ref.visits), (what, got.tokens, got.oov, got.visits, ref.tokens, ref.oov, ref.visits)
    for m, (a, b) in enumerate(zip(got.z, ref.z)):
        assert (a is None) == (b is None), (what, m)
        if a is not None:
            assert a.dtype == np.int32 and np.array_equal(a, b), (what, m, np.flatnonzero(a != b)[:8])
    assert got.counts_sum.dtype == np.int32 and np.array_equal(got.counts_sum, ref.counts_sum), what
    assert got.theta.dtype == np.float64 and np.array_equal(got.theta.view(np.uint64), ref.theta.view(np.uint64)), \
        (what, np.argwhere(got.theta != ref.theta)[:8])


ASYM = np.array([[1.0, 0.3, 0.0], [0.6, 0.8, 0.25], [0.05, 0.0, 1.5]])         # a caller's coupling: asymmetric, zeros, a diagonal that is not 1


@pytest.mark.parametrize("run", [dict(iterations=3), dict(iterations=7, samples=3, thin=2)], ids=["plain", "samples"])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("K", KS)
def test_shapes_equal_the_restatement(models, K, M, run):
    mdl = models(K, M)
    offs, toks = fc.foldin_docs(mdl.V, n_docs=40, seed=K + M)
    assert set(np.diff(offs[0])) == set(fc.LENGTHS)
    frozen = mdl.frozen()
    for coupling in ((None,) if M == 1 else (None, ASYM)):
        ref = fr.run(frozen, offs, toks, mdl.w, seed=1234 + K, doc_base=7, coupling=coupling, **run)
        got = mdl.s.fold_in(offs, toks, mdl.w, seed=1234 + K, doc_base=7, coupling=coupling, want_z=True, want_counts=True, **run)
        assert ref.oov > 0 and ref.visits == ref.tokens * run["iterations"] and got.kernel_ms > 0
        assert_equals_ref(got, ref, (K, M, run, coupling is not None))


def test_a_view_no_document_has(models):
    mdl = models(100, 3)
    offs, toks = fc.foldin_docs(mdl.V, n_docs=20, seed=4, null_view=1)
    assert offs[1] is None
    ref = fr.run(mdl.frozen(), offs, toks, mdl.w, iterations=3, seed=9)
    got = mdl.s.fold_in(offs, toks, mdl.w, iterations=3, seed=9, want_z=True, want_counts=True)
    assert got.z[1] is None and not got.counts_sum[:, 1].any()
    assert_equals_ref(got, ref, "null view")


def test_the_largest_footprint_eight_views_2048_topics():
    K, V = 2048, [40, 12, 12, 12, 12, 12, 12, 12]
    rng = np.random.default_rng(5)
    hy = hyper(K, V, 5)
    nwk = [rng.integers(0, 4, (v, K)).astype(np.int32) for v in V]
    offs = [np.array([0, 5, 5, 9, 12], dtype=np.int64) if m % 2 == 0 else np.array([0, 0, 3, 4, 10], dtype=np.int64) for m in range(8)]
    toks = [rng.integers(0, V[m] + 2, offs[m][-1]).astype(np.int32) for m in range(8)]
    w = np.linspace(1.0, 0.3, 8)
    with NativeSampler(K, V) as s:
        s.set_hyper(hy)
        for m in range(8):
            s.set_counts(m, nwk[m], nwk[m].sum(0).astype(np.int32))
        frozen = fr.Model(nwk, np.stack([x.sum(0) for x in nwk]), hy.beta, hy.beta_sum, hy.gamma, hy.alpha[:, :K], hy.alpha_sum, None, hy.p_a, hy.p_b)
        ref = fr.run(frozen, offs, toks, w, iterations=3, samples=2, thin=1, seed=3)
        got = s.fold_in(offs, toks, w, iterations=3, samples=2, thin=1, seed=3, want_z=True, want_counts=True)
        assert_equals_ref(got, ref, "M = 8, K = 2048")


def test_a_long_document_keeps_z_beyond_the_lds_cap(models):
    mdl = models(100, 3)
    rng = np.random.default_rng(6)
    offs = [np.array([0, 600], dtype=np.int64), np.array([0, 5], dtype=np.int64), np.array([0, 0], dtype=np.int64)]
    toks = [rng.integers(0, mdl.V[0], 600).astype(np.int32), rng.integers(0, mdl.V[1], 5).astype(np.int32), np.zeros(0, dtype=np.int32)]
    toks[0][[0, 300, 511, 512, 555, 599]] = mdl.V[0]                          # out of vocabulary on both sides of the cap; view 1 lies beyond it
    ref = fr.run(mdl.frozen(), offs, toks, mdl.w, iterations=4, samples=2, thin=1, seed=5)
    assert ref.visits == 4 * (594 + 5)
    got = mdl.s.fold_in(offs, toks, mdl.w, iterations=4, samples=2, thin=1, seed=5, want_z=True, want_counts=True)
    assert_equals_ref(got, ref, "long")


def test_more_documents_than_waves_go_through_the_queue(models):
    mdl = models(64, 1)
    rng = np.random.default_rng(8)
    lens = rng.integers(0, 9, 300)
    offs = [np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)]
    toks = [rng.integers(0, mdl.V[0] + 10, offs[0][-1]).astype(np.int32)]      # some out of vocabulary
    ref = fr.run(mdl.frozen(), offs, toks, mdl.w, iterations=5, seed=77)
    got = mdl.s.fold_in(offs, toks, mdl.w, iterations=5, seed=77, want_z=True, want_counts=True)   # 300 documents, eight a block
    assert_equals_ref(got, ref, "queue")


def test_theta_is_doc_topic_proportions_of_the_returned_assignments(models):
    for K, M in ((100, 3), (130, 1)):
        mdl = models(K, M)
        offs, toks = fc.foldin_docs(mdl.V, n_docs=30, seed=21)
        got = mdl.s.fold_in(offs, toks, mdl.w, iterations=3, seed=2, want_z=True)
        with NativeSampler(K, mdl.V) as s2:
            for m in range(M):
                s2.set_corpus(m, offs[m], np.minimum(toks[m], mdl.V[m] - 1))      # (the proportions read lengths and z, never the tokens)
                s2.set_view_presence(m, np.ones(30, dtype=np.uint8))
                s2.set_assignments(m, got.z[m])
            s2.set_hyper(mdl.hy)
            want = s2.doc_topic_proportions(mdl.w)
        assert np.array_equal(got.theta.view(np.uint64), want.view(np.uint64)), np.argwhere(got.theta != want)[:8]


@pytest.fixture(scope="module")
def peaked():
    s = NativeSampler(3, [2])
    hy = Hyper.defaults(3, [2], alpha=0.05, beta=fc.PEAKED_BETA)
    hy.alpha[0, :3] = fc.PEAKED_ALPHA
    hy.alpha_sum[0] = fc.PEAKED_ALPHA_SUM
    hy.gamma[0] = fc.PEAKED_GAMMA
    s.set_hyper(hy)
    s.set_counts(0, fc.PEAKED_NWK, fc.PEAKED_NK)
    yield s
    s.close()


def test_one_token_documents_follow_the_exact_distribution_on_the_device(peaked):
    p, half, prior = fc.peaked_expectation()
    off, tok = fc.peaked_docs()
    got = peaked.fold_in(off, tok, None, iterations=1, seed=11, doc_base=1000, want_z=True)
    freq = fc.frequencies(got.z[0])
    print("frequencies", freq, "exact", p, "half-widths", half)
    assert got.theta is None and (np.abs(freq - p) <= half).all() and (np.abs(prior - p) > half).any()
    ref = fr.run(fc.peaked_model(), off, tok, iterations=1, seed=11, doc_base=1000)
    assert np.array_equal(got.z[0], ref.z[0])


def test_two_calls_same_bytes_and_nothing_of_the_handle_moves(models):
    mdl = models(130, 3)
    s = mdl.s
    offs, toks = fc.foldin_docs(mdl.V, n_docs=20, seed=2)
    before = [s.get_counts(m) for m in range(3)], [s.get_assignments(m) for m in range(3)], s.trees_current(), s.counts_written(), bytes(s.get_tuning())
    one = s.fold_in(offs, toks, mdl.w, iterations=3, seed=8, want_z=True, want_counts=True)
    two = s.fold_in(offs, toks, mdl.w, iterations=3, seed=8, want_z=True, want_counts=True)
    assert one.theta.tobytes() == two.theta.tobytes() and one.counts_sum.tobytes() == two.counts_sum.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one.z, two.z))
    assert (one.tokens, one.oov, one.visits) == (two.tokens, two.oov, two.visits)
    other = s.fold_in(offs, toks, mdl.w, iterations=3, seed=9, want_z=True)
    assert other.theta.tobytes() != one.theta.tobytes()                      # the seed reaches the draws
    after = [s.get_counts(m) for m in range(3)], [s.get_assignments(m) for m in range(3)], s.trees_current(), s.counts_written(), bytes(s.get_tuning())
    for m in range(3):
        assert np.array_equal(before[0][m][0], after[0][m][0]) and np.array_equal(before[0][m][1], after[0][m][1])
        assert np.array_equal(before[1][m], after[1][m])
    assert before[2:] == after[2:]


def test_a_document_does_not_depend_on_its_batch(models):
    mdl = models(100, 3)
    offs, toks = fc.foldin_docs(mdl.V, n_docs=40, seed=14)
    whole = mdl.s.fold_in(offs, toks, mdl.w, iterations=3, samples=2, seed=4, doc_base=100, want_z=True, want_counts=True)
    so, st = fc.slice_docs(offs, toks, 10, 30)
    part = mdl.s.fold_in(so, st, mdl.w, iterations=3, samples=2, seed=4, doc_base=110, want_z=True, want_counts=True)
    assert part.theta.tobytes() == whole.theta[10:30].tobytes() and np.array_equal(part.counts_sum, whole.counts_sum[10:30])
    for m in range(3):
        assert np.array_equal(part.z[m], whole.z[m][offs[m][10]:offs[m][30]])


def raw_call(s, args, D, offs, toks, theta, z, cs):
    vpM = C.c_void_p * s.M
    st = _lib.FoldinStatsC(-7, -7, -7, -7.0)
    rc = s.L.mvhdp_fold_in(s.h, C.byref(args), D, vpM(*[o.ctypes.data for o in offs]), vpM(*[t.ctypes.data for t in toks]), theta.ctypes.data,
                           vpM(*[x.ctypes.data for x in z]), cs.ctypes.data, C.byref(st))
    return rc, st


def test_error_paths_leave_every_output_untouched(models):
    mdl = models(5, 1)
    K = 5
    off = np.array([0, 2, 3], dtype=np.int64)
    tok = np.array([1, 2, 3], dtype=np.int32)
    w = np.array([1.0])

    def untouched(s, code, off=off, tok=tok, w=w, iterations=3, samples=1, thin=1, coupling=None, doc_base=0):
        a = _lib.FoldinArgsC(iterations, samples, thin, 5, doc_base, None if coupling is None else coupling.ctypes.data, None if w is None else w.ctypes.data)
        theta, z, cs = np.full((2, K), -7.0), [np.full(len(tok), -7, dtype=np.int32)], np.full((2, 1, K), -7, dtype=np.int32)
        rc, st = raw_call(s, a, 2, [off], [tok], theta, z, cs)
        assert rc == code, (rc, code, s.L.mvhdp_last_error(s.h))
        assert (theta == -7).all() and (z[0] == -7).all() and (cs == -7).all() and (st.tokens, st.oov, st.visits, st.kernel_ms) == (-7, -7, -7, -7.0)

    with NativeSampler(K, mdl.V) as fresh:                                   # no counts yet
        fresh.set_hyper(mdl.hy)
        untouched(fresh, STATE)
    with NativeSampler(K, mdl.V) as fresh:                                   # counts, no hyper-parameters
        nwk, nk = mdl.s.get_counts(0)
        fresh.set_counts(0, nwk, nk)
        untouched(fresh, STATE)
    s = mdl.s
    untouched(s, INV, tok=np.array([1, -2, 3], dtype=np.int32))              # a negative token
    untouched(s, INV, off=np.array([0, 3, 2], dtype=np.int64))               # doc_off goes down
    untouched(s, INV, off=np.array([1, 2, 3], dtype=np.int64))               # ... or does not start at 0
    untouched(s, INV, iterations=0)
    untouched(s, INV, iterations=65536)
    untouched(s, INV, iterations=4, samples=3, thin=2)                       # the first recorded iteration would be 0
    untouched(s, INV, samples=0)
    untouched(s, INV, thin=0)
    untouched(s, INV, doc_base=-1)
    untouched(s, INV, coupling=np.array([np.nan]))
    untouched(s, INV, coupling=np.array([-0.5]))
    untouched(s, INV, w=np.array([-1.0]))
    untouched(s, INV, w=np.array([0.0]))
    untouched(s, INV, w=np.array([np.inf]))
    untouched(s, INV, w=None)                                                # theta asked for without weights
    with pytest.raises(MvhdpError) as e:
        s.fold_in([off], [tok], w, iterations=0)
    assert e.value.code == INV and "iterations" in str(e.value)
    # the same buffers with good arguments are written; a NULL theta with NULL view_weights is accepted
    a = _lib.FoldinArgsC(3, 1, 1, 5, 0, None, w.ctypes.data)
    theta, z, cs = np.full((2, K), -7.0), [np.full(3, -7, dtype=np.int32)], np.full((2, 1, K), -7, dtype=np.int32)
    rc, st = raw_call(s, a, 2, [off], [tok], theta, z, cs)
    assert rc == 0 and not (theta == -7).any() and not (z[0] == -7).any() and not (cs == -7).any() and (st.tokens, st.oov, st.visits) == (3, 0, 9)
    none = s.fold_in([off], [tok], None, iterations=3, seed=5, want_z=True)
    assert none.theta is None and np.array_equal(none.z[0], z[0])
    empty = s.fold_in([np.array([0], dtype=np.int64)], [np.zeros(0, dtype=np.int32)], w)
    assert empty.theta.shape == (0, K) and (empty.tokens, empty.visits) == (0, 0)


def test_theta_chains_into_nearest_entities_and_predict_items(models):
    mdl = models(100, 3)
    s = mdl.s
    offs, toks = fc.foldin_docs(mdl.V, n_docs=12, seed=31, lengths=[0, 1, 2, 9, 40])
    r = s.fold_in(offs, toks, mdl.w, iterations=5, seed=3)
    rows = np.array(r.theta.tolist(), dtype=np.float64)                      # the same rows from numpy's side
    near, want = s.nearest_entities(mdl.w, 5, queries=r.theta), s.nearest_entities(mdl.w, 5, queries=rows)
    assert np.array_equal(near.ids, want.ids) and near.sims.tobytes() == want.sims.tobytes() and (near.counts == 5).all()
    items, scores, counts = s.predict_items(1, None, 4, 0, 12, exclude_present=False, theta=r.theta)
    items2, scores2, counts2 = s.predict_items(1, None, 4, 0, 12, exclude_present=False, theta=rows)
    assert np.array_equal(items, items2) and scores.tobytes() == scores2.tobytes() and np.array_equal(counts, counts2) and (counts == 4).all()


def test_group_of_two_members_equals_one_handle(models):
    mdl = models(100, 3)
    offs, toks = fc.foldin_docs(mdl.V, n_docs=16, seed=12)
    one = mdl.s.fold_in(offs, toks, mdl.w, iterations=3, seed=31, doc_base=5, want_z=True, want_counts=True)
    members = []
    try:
        for _ in range(2):                                                   # every member holds the full counts
            s = NativeSampler(mdl.K, mdl.V)
            s.set_hyper(mdl.hy)
            for m in range(3):
                s.set_counts(m, *mdl.s.get_counts(m))
            members.append(s)
        g = NativeGroup.__new__(NativeGroup)                                 # (no collective is needed for this: the local members, as topic_phrases)
        g.members, g.g = members, None
        two = g.fold_in(offs, toks, mdl.w, iterations=3, seed=31, doc_base=5, want_z=True, want_counts=True)
        assert two.theta.tobytes() == one.theta.tobytes() and np.array_equal(two.counts_sum, one.counts_sum)
        assert all(np.array_equal(a, b) for a, b in zip(two.z, one.z)) and (two.tokens, two.oov, two.visits) == (one.tokens, one.oov, one.visits)
    finally:
        for s in members:
            s.close()
