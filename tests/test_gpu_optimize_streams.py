"""The optimize steps' stochastic kernels (mvhdp_stats.hip: gamma_doc_stats_kernel, dp_tables_kernel, antoniak_draws_kernel) against
the oracle's restatements of their stream contract (oracle/mvhdp_oracle.c, pinned on the CPU by tests/test_optimize_streams_kats.py),
draw for draw; and the deterministic statistics of the steps either side of the sweep at the shapes where their kernels change path
(LDS vs global atomics, dynamic LDS sizes, grid wrap, histogram cut-offs, carried-over entities).

qs, mk, active and tables are integers and must be equal.  qw is a sum of log Beta(gamma + 1, j) terms built from the device's
log, cos and sqrt (OCML), which are not glibc's: the Marsaglia-Tsang values then differ in their last bits, never in which
proposal is accepted (a flip would move a term by O(0.1), not by 1e-13).  So qw is compared with a tolerance: relative 1e-13,
plus a few ulps of 1 per entity, because log(ga / (ga + gb)) is an absolute, not a relative, function of the quotient's error (a
term near 0 at gamma = 1e4 keeps its absolute error, not its relative one)."""
import ctypes as C

import numpy as np
import pytest

from mvtopicmodel_amd import NativeGroup, NativeSampler
from mvtopicmodel_amd._lib import MvhdpError
from mvtopicmodel_amd.native import Hyper
from oracle import doc_topics
from oracle.binding import Oracle, antoniak_draws_philox, dp_tables_philox
from tests.helpers import make_native, make_oracle, small_corpus

pytestmark = pytest.mark.gpu

SEED = 0xA5A5_0001_DEAD_BEEF                   # high bits set: seed_hi enters every key
ROUNDS = (0, 15, 2**31 + 1)
CONCS = (0.0, 1e-300, 0.003, 1.7, 25.0, 1e12)
EPS = np.finfo(np.float64).eps
INVALID_ARG = -1


def _offs(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _pair(lens_per_view, doc_id_base=0, present=None):
    """A handle and an oracle model whose view m has entity lengths lens_per_view[m] (one vocabulary type): the optimize-step
    statistics read only the spans."""
    M = len(lens_per_view)
    s = NativeSampler(4, [1] * M, doc_id_base=doc_id_base)
    o = Oracle(4, [1] * M)
    for m, lens in enumerate(lens_per_view):
        off = _offs(lens)
        tok = np.zeros(int(off[-1]), dtype=np.int32)
        s.set_corpus(m, off, tok)
        o.set_corpus(m, off, tok)
    for m, p in (present or {}).items():
        s.set_view_presence(m, p)
    return s, o


def _qw_close(dev, ref, n_terms):
    return abs(dev - ref) <= 1e-13 * abs(ref) + 8 * EPS * n_terms


# ------------------------------------------------------------------------------------------------ dp_tables_kernel
def _hist(rng, K, L):
    """[K][L]: empty topics, topics with only i == 1, sparse cells of 0, 1, a few and 10^5 entities."""
    h = np.zeros((K, L), dtype=np.int32)
    h[:, 0] = rng.integers(0, 50, K)                                  # bucket 0 is never read
    if L == 1:
        return h
    kind = np.arange(K) % 4
    h[kind == 1, 1] = rng.integers(1, 9, int((kind == 1).sum()))    # only i == 1
    dense = max(1, min(L - 1, 3000 // max(K, 1) + 4))
    for t in np.flatnonzero(kind >= 2):
        cols = rng.integers(1, L, dense)
        h[t, cols] = rng.choice(np.array([1, 1, 2, 7, 100000], dtype=np.int32), dense)
    if K > 3:
        h[3, L - 1] = 1                                               # the last count, on the last stride-256 wrap
    return h


@pytest.mark.parametrize("K", [1, 2, 255, 256, 257, 2048])
def test_dp_table_statistics_equal_the_restatement(K):
    rng = np.random.default_rng(K)
    s = NativeSampler(K, [1] * 8)                                     # M = 8: view 7 is the last one
    conc = np.array([CONCS[(t + 3) % len(CONCS)] for t in range(K)], dtype=np.float64)   # K = 1, 2: real draws too
    if K > 5:
        conc[4], conc[5] = np.nan, -3.0
    for L in (1, 2, 257, 600):
        h = _hist(rng, K, L)
        for m in (0, 7):
            for rnd in ROUNDS if L == 600 else ROUNDS[1:2]:
                mk, act = s.dp_table_statistics(m, h, conc, SEED, rnd)
                rmk, ract = dp_tables_philox(h, conc, m, SEED, rnd)
                assert np.array_equal(act, ract), (L, m, rnd)
                assert np.array_equal(mk, rmk), (L, m, rnd, np.flatnonzero(mk != rmk)[:5])
    # the active rule by itself: held counts i >= 1 make a topic active whatever its concentration
    assert act.sum() == np.count_nonzero(h[:, 1:].max(axis=1) > 0)
    for bad in (dict(m=8), dict(m=-1), dict(L=0)):
        with pytest.raises(MvhdpError) as e:
            s.dp_table_statistics(bad.get("m", 0), np.zeros((K, bad.get("L", 4)), dtype=np.int32), conc, SEED, 0)
        assert e.value.code == INVALID_ARG
    s.close()


# ------------------------------------------------------------------------------------------------ antoniak_draws_kernel
@pytest.mark.parametrize("n", [1, 255, 256, 257, 200_000])
def test_antoniak_draws_equal_the_restatement(n):
    rng = np.random.default_rng(n)
    edges = np.array([-3, 0, 1, 2, 19999, 20000, 20001, 2**31 - 1], dtype=np.int32)
    items = rng.integers(1, 120, n).astype(np.int32)
    k = min(n, 64)
    items[rng.choice(n, k, replace=False)] = np.resize(edges, k)
    conc = np.asarray(CONCS, dtype=np.float64)[rng.integers(0, len(CONCS), n)]
    if n > 4:
        conc[1], conc[3] = np.nan, -1.0
    s = NativeSampler(4, [1])
    for rnd in ROUNDS:
        t = s.antoniak_draws(items, conc, SEED, rnd)
        r = antoniak_draws_philox(items, conc, SEED, rnd)
        assert np.array_equal(t, r), (rnd, np.flatnonzero(t != r)[:5])
    assert s.L.mvhdp_antoniak_draws(s.h, -1, None, None, 0, 0, None) == INVALID_ARG
    assert s.L.mvhdp_antoniak_draws(s.h, 3, None, None, 0, 0, None) == INVALID_ARG
    s.close()


# ------------------------------------------------------------------------------------------------ gamma_doc_stats_kernel
GAMMAS = (1e-3, 0.37, 1.0, 6.5, 1e4)


@pytest.mark.parametrize("j", [1, 2, 1_000_000])
def test_gamma_doc_statistics_of_one_entity(j):
    """D = 1: qs is the entity's Bernoulli bit, qw its term (the sum adds zeros only)."""
    s, o = _pair([[j]])
    for g in GAMMAS:
        for rnd in ROUNDS:
            qs, qw = s.gamma_doc_statistics(0, g, SEED, rnd)
            rqs, rqw, eb, ew = o.gamma_doc_stats_philox(0, g, SEED, rnd, per_entity=True)
            assert qs == rqs == float(eb[0]) and rqw == ew[0]
            assert _qw_close(qw, rqw, 1), (g, rnd, qw, rqw)
    s.close(); o.close()


def _corpus_lengths(rng, D, long_entity=False):
    lens = rng.poisson(3.0, D).astype(np.int64)
    lens[rng.random(D) < 0.1] = 0                                     # entities without the view
    if long_entity:
        lens[D // 3] = 1_000_000
    return lens


@pytest.mark.parametrize("D,base,long_entity", [(1, 0, False), (257, 17000, False), (262_144, 0, True), (262_145, 17000, False),
                                                (300_000, (1 << 29) - 300_001, False)])
def test_gamma_doc_statistics_equal_the_restatement(D, base, long_entity):
    """Entities wrap the 262 144-thread grid from D = 262 145 on; the last case puts the entity ids at the top of the range the
    API accepts.  View 1 has present-but-empty entities: skipped like the missing ones."""
    rng = np.random.default_rng(D)
    l0 = _corpus_lengths(rng, D, long_entity)
    l1 = _corpus_lengths(rng, D)
    present = (l1 > 0).astype(np.uint8)
    present[rng.random(D) < 0.05] = 1
    s, o = _pair([l0, l1], doc_id_base=base, present={1: present})
    for m, g, rnd in ((0, 0.37, 0), (1, 1.0, 15), (0, 1e4, 2**31 + 1), (1, 1e-3, 3), (0, 6.5, 7)):
        qs, qw = s.gamma_doc_statistics(m, g, SEED, rnd)
        rqs, rqw = o.gamma_doc_stats_philox(m, g, SEED, rnd, doc_id_base=base)
        nz = int(np.count_nonzero([l0, l1][m]))
        assert qs == rqs, (m, g, rnd)
        assert _qw_close(qw, rqw, nz), (m, g, rnd, qw, rqw, (qw - rqw) / rqw)
    s.close(); o.close()


def test_gamma_doc_statistics_entity_ids_above_2_to_32_are_refused():
    """The contract keys an entity's stream with seed_hi ^ (dg >> 32), but a handle's entity ids stay below 2^29
    (mvhdp_config.doc_id_base, set_corpus): the high word is 0 on the device, and the API says so."""
    with pytest.raises(MvhdpError):
        NativeSampler(4, [1], doc_id_base=2**32 + 5)
    s = NativeSampler(4, [1], doc_id_base=(1 << 29) - 4)
    with pytest.raises(MvhdpError):
        s.set_corpus(0, _offs([1, 1, 1, 1]), np.zeros(4, dtype=np.int32))
    s.close()


@pytest.mark.parametrize("n_shards", [2, 3])
def test_group_gamma_doc_statistics_is_the_sum_of_restated_shards(n_shards):
    K, V = 20, [200, 30]
    c = small_corpus(K, V, 900, [9, 2], 71)
    hy = Hyper.defaults(K, V)
    o = make_oracle(c, hy)
    z = [o.get_assignments(m) for m in range(2)]
    cuts = np.linspace(0, c.D, n_shards + 1).astype(int)
    shards, refs = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sub = c.slice_docs(int(lo), int(hi))
        shards.append(make_native(sub, hy, [zz[c.doc_off[m][lo]:c.doc_off[m][hi]] for m, zz in enumerate(z)], doc_id_base=int(lo)))
        r = Oracle(K, V)
        for m in range(2):
            r.set_corpus(m, sub.doc_off[m], sub.tokens[m])
        refs.append((r, int(lo)))
    with NativeGroup(shards) as g:
        for m, gm, rnd in ((0, 1.3, 0), (1, 0.37, 2**31 + 1)):
            qs, qw = g.gamma_doc_statistics(m, gm, SEED, rnd)
            parts = [r.gamma_doc_stats_philox(m, gm, SEED, rnd, doc_id_base=lo) for r, lo in refs]
            assert qs == sum(p[0] for p in parts)
            want = sum(p[1] for p in parts)
            assert abs(qw - want) <= 1e-12 * abs(want), (qw, want)
            whole = o.gamma_doc_stats_philox(m, gm, SEED, rnd)         # the same entities' draws as the unsharded model
            assert qs == whole[0]
    for sh in shards:
        sh.close()
    for r, _ in refs:
        r.close()
    o.close()


# ------------------------------------------------------------------------------------------------ deterministic statistics at their edges
def test_count_histogram_around_the_lds_cut():
    """count_hist_kernel counts c < 1024 in LDS and c >= 1024 with global atomics; K = 1, V = 1 is a one-cell model."""
    s = NativeSampler(1, [1])
    s.set_corpus(0, _offs([1]), np.zeros(1, dtype=np.int32))
    for c in (1, 1023, 1024, 1025, 70_000):
        s.set_counts(0, np.array([[c]], dtype=np.int32), np.array([c], dtype=np.int32))
        for n in (1, 2, 1000, 1024, 1025, c + 1):
            h = s.get_count_histogram(0, n)
            want = np.bincount([c], minlength=n)[:n] if c < n else np.zeros(n, dtype=np.int64)
            want[0] = 0
            assert np.array_equal(h, want), (c, n)
    s.close()
    # many cells straddling the cut, K = 7, V = 500
    rng = np.random.default_rng(3)
    K, V = 7, 500
    s = NativeSampler(K, [V])
    s.set_corpus(0, _offs([1]), np.zeros(1, dtype=np.int32))
    nwk = rng.choice(np.array([0, 1, 5, 1023, 1024, 1025, 4097, 70_000], dtype=np.int32), (V, K))
    s.set_counts(0, nwk, nwk.sum(axis=0).astype(np.int32))
    for n in (1, 1024, 1025, 70_001):
        want = np.bincount(nwk.ravel(), minlength=n)[:n]
        want[0] = 0
        assert np.array_equal(s.get_count_histogram(0, n), want), n
    s.close()


def _recount_doc_topic_hist(K, off, z, hist_len, len_len, present=None):
    D = len(off) - 1
    hist = np.zeros((K, hist_len), dtype=np.int64)
    dl = np.zeros(len_len, dtype=np.int64)
    ks = np.arange(K)
    for d in range(D):
        b, e = off[d], off[d + 1]
        if e == b and (present is None or not present[d]):
            continue
        if e - b < len_len:
            dl[e - b] += 1
        n = np.bincount(z[b:e][z[b:e] >= 0], minlength=K)
        keep = n < hist_len                                             # bucket 0: entities with the view not holding k
        hist[ks[keep], n[keep]] += 1
    return hist, dl


@pytest.mark.parametrize("K", [1, 512, 513, 1200, 2048])
def test_doc_topic_hist_at_its_shapes(K):
    rng = np.random.default_rng(K)
    D = 300
    lens = rng.poisson(12, D).astype(np.int64)
    lens[::17] = 0
    lens[5] = 700                                                     # the longest entity
    off = _offs(lens)
    z = rng.integers(0, min(K, 6), int(off[-1])).astype(np.int32)   # few topics: counts per entity run high
    z[rng.random(len(z)) < 0.02] = -1                                 # unassigned tokens
    s = NativeSampler(K, [3])
    s.set_corpus(0, off, np.zeros(int(off[-1]), dtype=np.int32))
    s.set_assignments(0, z)
    o = Oracle(K, [3])
    o.set_corpus(0, off, np.zeros(int(off[-1]), dtype=np.int32))
    o.set_assignments(0, z)
    for hl, ll in ((2, 3), (40, 701)):
        h, dl = s.get_doc_topic_hist(0, hl, ll)
        oh, odl = o.get_doc_topic_hist(0, hl, ll)
        wh, wd = _recount_doc_topic_hist(K, off, z, hl, ll)
        assert np.array_equal(h, oh) and np.array_equal(h, wh) and np.array_equal(dl, odl) and np.array_equal(dl, wd)
    o.close()
    present = (lens > 0).astype(np.uint8)
    present[::34] = 1                                                 # present but empty
    s.set_view_presence(0, present)
    topmax = int(max(np.bincount(z[off[d]:off[d + 1]][z[off[d]:off[d + 1]] >= 0], minlength=K).max() for d in range(D) if lens[d]))
    for hl, ll in ((1, 1), (3, 5), (topmax, 700), (topmax + 1, 701), (800, 900)):   # hl <= topmax: holders beyond the cut
        h, dl = s.get_doc_topic_hist(0, hl, ll)
        wh, wd = _recount_doc_topic_hist(K, off, z, hl, ll, present)
        assert np.array_equal(h, wh), (hl, ll)
        assert np.array_equal(dl, wd), (hl, ll)
    # NULL outputs through the C ABI
    h = np.zeros((K, 4), dtype=np.int32)
    assert s.L.mvhdp_get_doc_topic_hist(s.h, 0, h.ctypes.data_as(C.c_void_p), 4, None, 0) == 0
    assert np.array_equal(h, _recount_doc_topic_hist(K, off, z, 4, 1, present)[0])
    dl = np.zeros(9, dtype=np.int32)
    assert s.L.mvhdp_get_doc_topic_hist(s.h, 0, None, 0, dl.ctypes.data_as(C.c_void_p), 9) == 0
    assert np.array_equal(dl, _recount_doc_topic_hist(K, off, z, 1, 9, present)[1])
    assert s.L.mvhdp_get_doc_topic_hist(s.h, 0, h.ctypes.data_as(C.c_void_p), 0, None, 0) == INVALID_ARG
    s.close()


def _random_model(K, lens, rng, V=5, unassigned=0.0):
    """A handle and an oracle model with entity lengths lens[m][d], random types and topics (a fraction unassigned)."""
    M = len(lens)
    s, o = NativeSampler(K, [V] * M), Oracle(K, [V] * M)
    offs, zs, toks = [], [], []
    for m in range(M):
        off = _offs(lens[m])
        tok = rng.integers(0, V, int(off[-1])).astype(np.int32)
        z = rng.integers(0, K, int(off[-1])).astype(np.int32)
        z[rng.random(len(z)) < unassigned] = -1
        offs.append(off); zs.append(z); toks.append(tok)
    return s, o, offs, zs, toks


def _load(s, o, offs, zs, toks, hy=None):
    for m, (off, z, tok) in enumerate(zip(offs, zs, toks)):
        for x in (s, o):
            x.set_corpus(m, off, tok)
            x.set_assignments(m, z)
    if hy is not None:
        s.set_hyper(hy)
        o.set_hyper(hy.alpha, hy.alpha_sum, hy.beta, hy.beta_sum, hy.gamma, hy.p_a, hy.p_b, hy.inactive)


def _proportions_case(K, lens, seed, windows):
    rng = np.random.default_rng(seed)
    M = len(lens)
    s, o, offs, zs, toks = _random_model(K, lens, rng, unassigned=0.05)
    hy = Hyper.defaults(K, [5] * M)
    hy.alpha[:, :K] = rng.uniform(0.01, 0.3, (M, K)); hy.alpha_sum[:] = hy.alpha[:, :K].sum(axis=1)
    hy.gamma[:] = rng.uniform(0.5, 2.0, M)
    _load(s, o, offs, zs, toks, hy)
    w = rng.uniform(0.1, 1.5, M); w[0] = 1.0
    ref = doc_topics.doc_topic_proportions(K, offs, zs, hy.alpha, hy.alpha_sum, hy.gamma, w)
    assert np.array_equal(s.doc_topic_proportions(w), ref)
    for d0, d1 in windows:
        assert np.array_equal(s.doc_topic_proportions(w, d0, d1), ref[d0:d1]), (d0, d1)
    s.close(); o.close()


def test_doc_topic_proportions_at_64_kib_and_carried_windows():
    """M = 8, K = 2048: M*K ints of dynamic LDS are exactly 64 KiB.  Windows start right after entities lacking views, so the
    window's first entities are scored with counts of a holder before d0 (PTM:2873-2886)."""
    K, M, D = 2048, 8, 120
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 30, (M, D))
    lens[1:, 10:14] = 0                                               # entities 10..13 have view 0 only
    lens[:, 40] = 0; lens[4, 40] = 3
    lens[3, 0] = 0                                                    # view 3 missing on entity 0: zeros, no holder yet
    _proportions_case(K, lens, 5, [(11, 20), (12, 13), (41, 60), (0, 1), (119, 120), (7, 7)])


def test_doc_topic_proportions_beyond_the_grid():
    """D above the 16 384 workgroups of doc_topic_prop_kernel: workgroups take a second entity."""
    K, M, D = 24, 2, 16384 + 611
    rng = np.random.default_rng(6)
    lens = rng.integers(0, 6, (M, D))
    _proportions_case(K, lens, 6, [(100, D), (16383, 16385)])


def test_view_overlap_sums_at_eight_views_and_every_bitmap_word():
    """M = 8 with equal view lengths (the TreeMap keeps the later view, PTM:2741) and entities with one view only; K = 2048 with
    topics in every one of the 64 words of an entity's bitmap."""
    K, M, D = 2048, 8, 200
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 40, (M, D))
    lens[:, :40] = 9                                                  # equal lengths in every view
    lens[1:, 40:60] = 0                                               # view 0 only
    lens[:, 60] = 0; lens[3, 60] = 12                                 # one middle view only
    lens[:, 61] = 64; lens[:, 62] = 200
    s, o, offs, zs, toks = _random_model(K, lens, rng)
    for m in range(M):
        b = offs[m][62]
        zs[m][b:b + 64] = np.arange(64) * 32 + m                      # entity 62: a topic in every bitmap word
    _load(s, o, offs, zs, toks)
    assert np.array_equal(s.view_overlap_sums(), o.optimize_p_sums())
    s.close(); o.close()


def test_model_log_likelihood_at_k2048_m8():
    """Entities of length 0, 1 and 2 (backing-array phantom tokens), unassigned tokens and one entity longer than 64 K."""
    K, M, D = 2048, 8, 90
    rng = np.random.default_rng(12)
    lens = rng.integers(0, 4, (M, D))
    lens[0, 7] = 64 * K + 5
    s, o, offs, zs, toks = _random_model(K, lens, rng, V=30, unassigned=0.1)
    _load(s, o, offs, zs, toks, Hyper.defaults(K, [30] * M))
    s.build_counts()
    o.build_counts()
    ll, ref = s.model_log_likelihood(), o.model_log_likelihood()
    assert np.allclose(ll, ref, rtol=1e-12, atol=0), (ll, ref)
    s.close(); o.close()
