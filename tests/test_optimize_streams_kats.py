"""The oracle's restatements of the optimize steps' device streams (oracle/mvhdp_oracle.c: orc_gamma_doc_stats_philox,
orc_dp_tables_philox, orc_antoniak_draws_philox), pinned on the CPU so that the GPU tests of tests/test_gpu_optimize_streams.py
can compare the kernels against them integer for integer.  Three kinds of check:
  * wiring: the first uniforms of a cell / draw / entity rebuilt here from the raw Philox words, and a full Python restatement of
    one entity's Marsaglia-Tsang draws (same libm as the oracle, so equal bits);
  * distributions, with many more draws than a GPU test can afford: the Antoniak closed forms and the Stirling pmf, the
    digamma / trigamma forms of log Beta(gamma + 1, j), in every Marsaglia-Tsang shape regime the kernel meets;
  * independence: every counter and key field separates streams, and sharding the entities changes no entity's draws."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import binding
from oracle.binding import Oracle, antoniak_draws_philox, dp_tables_philox


def _philox(ctr, key):
    L = binding.lib()
    c = (C.c_uint32 * 4)(*[x & 0xFFFFFFFF for x in ctr])
    k = (C.c_uint32 * 2)(*[x & 0xFFFFFFFF for x in key])
    o = (C.c_uint32 * 4)()
    L.orc_philox4x32_10(c, k, o)
    return list(o)


def _unit(hi, lo):
    return float(((hi << 32) | lo) >> 11) * 2.0 ** -53


class _Stream:
    """PhiloxStream::uniform from the raw words: call c0 = 0, 1, ... gives (x0,x1) then (x2,x3)."""

    def __init__(self, c1, c2, c3, k0, k1):
        self.c, self.k, self.buf = [0, c1, c2, c3], [k0, k1], []

    def uniform(self):
        if not self.buf:
            x = _philox(self.c, self.k)
            self.c[0] += 1
            self.buf = [_unit(x[0], x[1]), _unit(x[2], x[3])]
        return self.buf.pop(0)


def _mt_gamma(r, a):
    d = a - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    while True:
        u1, u2 = r.uniform(), r.uniform()
        if u1 <= 0.0:
            u1 = 2.0 ** -53
        n = math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
        t = 1.0 + c * n
        if t <= 0.0:
            continue
        v = t * t * t
        u = r.uniform()
        if u <= 0.0:
            u = 2.0 ** -53
        if u < 1.0 - 0.0331 * (n * n) * (n * n):
            return d * v
        if math.log(u) < 0.5 * n * n + d * (1.0 - v + math.log(v)):
            return d * v


def _lengths_oracle(lens, M=1):
    """An oracle model whose view m has entity lengths lens[m] (tokens all type 0): only the spans matter here."""
    lens = [np.asarray(x, dtype=np.int64) for x in (lens if M > 1 else [lens])]
    o = Oracle(2, [1] * len(lens))
    for m, ln in enumerate(lens):
        off = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
        o.set_corpus(m, off, np.zeros(int(off[-1]), dtype=np.int32))
    return o


SEED = 0xA5A5_0001_DEAD_BEEF                  # high bits set: seed_hi enters every key


# ---------------------------------------------------------------------------- wiring
@pytest.mark.parametrize("m,t,i,rnd,a", [(0, 0, 2, 0, 1.7), (7, 2047, 9, 15, 0.37), (3, 513, 40, 2**31 + 1, 25.0)])
def test_dp_tables_cell_stream_by_hand(m, t, i, rnd, a):
    K = t + 1
    hist = np.zeros((K, i + 1), dtype=np.int32)
    hist[t, i] = 3
    r = _Stream(0x300 + m, t, i, (SEED & 0xFFFFFFFF) ^ rnd, SEED >> 32)
    tables = 1 + sum(1 for l in range(1, i) if r.uniform() * (a + l) < a)
    conc = np.full(K, a)
    mk, act = dp_tables_philox(hist, conc, m, SEED, rnd)
    assert mk[t] == 3.0 * tables and act[t] == 1
    assert not mk[:t].any() and not act[:t].any()
    conc[t] = 1e300                                                   # every table opens: exactly i
    assert dp_tables_philox(hist, conc, m, SEED, rnd)[0][t] == 3.0 * i
    for c in (0.0, -2.5, float("nan")):                               # no concentration: one table per cell
        conc[t] = c
        mk, act = dp_tables_philox(hist, conc, m, SEED, rnd)
        assert mk[t] == 3.0 and act[t] == 1


def test_dp_tables_cell_kinds():
    hist = np.zeros((4, 6), dtype=np.int32)
    hist[0, 1] = 7                                                    # i == 1: one table per entity, no draw
    hist[1, 0] = 5                                                    # bucket 0 alone: not active, nothing counted
    hist[2, 3] = -4                                                   # a negative cell counts as empty
    hist[3, 5] = 100000
    mk, act = dp_tables_philox(hist, np.full(4, 1e300), 0, 1, 0)
    assert list(mk) == [7.0, 0.0, 0.0, 500000.0] and list(act) == [1, 0, 0, 1]
    mk, act = dp_tables_philox(hist[:, :1], np.ones(4), 0, 1, 0)     # hist_len 1: no count is held at all
    assert not mk.any() and not act.any()


@pytest.mark.parametrize("j,it,a,rnd", [(0, 2, 1.3, 0), (5, 17, 0.003, 9), (256, 300, 6.0, 2**31 + 1)])
def test_antoniak_draw_stream_by_hand(j, it, a, rnd):
    items = np.full(j + 1, 1, dtype=np.int32)
    items[j] = it
    conc = np.full(j + 1, a)
    r = _Stream(0x400, j, rnd, SEED & 0xFFFFFFFF, SEED >> 32)
    want = 1 + sum(1 for l in range(1, it) if r.uniform() * (a + l) < a)
    got = antoniak_draws_philox(items, conc, SEED, rnd)
    assert got[j] == want and np.all(got[:j] == 1)


def test_antoniak_edges():
    items = np.array([-3, 0, 1, 2, 19999, 20000, 20001, 2**31 - 1], dtype=np.int32)
    for a, lo_one in ((1e300, False), (0.0, True), (-1.0, True), (float("nan"), True), (1e-300, True)):
        t = antoniak_draws_philox(items, np.full(len(items), a), 3, 1)
        assert list(t[:3]) == [0, 0, 1] and list(t[6:]) == [1, 1]      # beyond MAXSTIRLING = 20000: one table
        if lo_one:
            assert list(t[3:6]) == [1, 1, 1]                            # 1e-300: a / (a + l) rounds u (a + l) < a to u < 1e-300 / l
        else:
            assert list(t[3:6]) == [2, 19999, 20000]


@pytest.mark.parametrize("base", [0, 17000, 2**32 + 5])
def test_gamma_entity_stream_by_hand(base):
    """The first uniform decides the Bernoulli; then Gamma(gamma + 1) and Gamma(j) from the same stream.  The Python restatement
    calls the same libm as the oracle in the same order, so the per-entity qw terms agree bit for bit."""
    lens = np.array([3, 0, 1, 2, 50, 7, 1000, 0, 4], dtype=np.int64)
    o = _lengths_oracle(lens)
    for g, rnd in ((0.37, 0), (1e-3, 15), (6.5, 2**31 + 1), (1e4, 3)):
        qs, qw, eb, ew = o.gamma_doc_stats_philox(0, g, SEED, rnd, doc_id_base=base, per_entity=True)
        for d, j in enumerate(lens):
            if j == 0:
                assert eb[d] == 0 and ew[d] == 0.0
                continue
            dg = base + d
            r = _Stream(0x200, dg & 0xFFFFFFFF, rnd, SEED & 0xFFFFFFFF, (SEED >> 32) ^ (dg >> 32))
            assert eb[d] == (r.uniform() < j / (j + g))
            ga = _mt_gamma(r, g + 1.0)
            gb = _mt_gamma(r, float(j))
            assert ew[d] == math.log(ga / (ga + gb)), (d, g)
        assert qs == eb.sum() and math.isclose(qw, ew.sum(), rel_tol=1e-14)
    o.close()


def test_gamma_sum_order_is_the_device_grid():
    """qw is summed per thread (entity d on thread d mod 262144), then the 256-thread block tree, then the blocks in order: at
    D = 300 000 the first 37 856 threads hold two entities each."""
    rng = np.random.default_rng(4)
    D = 300_000
    lens = rng.integers(1, 6, D)
    o = _lengths_oracle(lens)
    qs, qw, eb, ew = o.gamma_doc_stats_philox(0, 0.8, 77, 2, per_entity=True)
    nt = 1024 * 256
    th = ew[:nt].copy()                                               # the per-thread running sums, in entity order
    th[:D - nt] += ew[nt:]
    sh = th.reshape(1024, 256).copy()
    s = 128
    while s >= 1:
        sh[:, :s] += sh[:, s:2 * s]
        s >>= 1
    want = 0.0
    for b in range(1024):
        want += sh[b, 0]
    assert qw == want and qs == float(eb.sum())
    o.close()


# ---------------------------------------------------------------------------- distributions
def _antoniak_moments(a, n):
    l = np.arange(n, dtype=np.float64)
    return (a / (a + l)).sum(), (a * l / (a + l) ** 2).sum()


@pytest.mark.parametrize("a,n", [(0.1, 50), (1.7, 12), (25.0, 63), (0.003, 2), (1e6, 30)])
def test_antoniak_distribution(a, n):
    from oracle import dp_samplers
    N = 200_000                                                       # the GPU moment test draws 4 000
    t = antoniak_draws_philox(np.full(N, n, dtype=np.int32), np.full(N, a), 11, 4).astype(np.float64)
    e, v = _antoniak_moments(a, n)
    assert 1 <= t.min() and t.max() <= n
    assert abs(t.mean() - e) < 4.5 * math.sqrt(v / N) + 1e-12, (t.mean(), e)
    if v * N > 2e4:                                                   # else too few non-trivial draws for a 5 % bound
        assert 0.95 * v < t.var() < 1.05 * v, (t.var(), v)
    row = np.array(dp_samplers.StaticSamplers().stirling(n), dtype=np.float64)   # the unscaled row of Samplers.java:1052-1084
    pmf = row * a ** np.arange(len(row)); pmf /= pmf.sum()
    got = np.bincount(t.astype(int), minlength=n + 1)[1:] / N
    sd = np.sqrt(pmf * (1 - pmf) / N)
    assert np.all(np.abs(got - pmf) <= 5 * sd + 1e-9), np.abs(got - pmf).max()


def test_dp_table_cells_follow_the_antoniak_law():
    """Cells of one count i across many topics, and across views and rounds, are independent Antoniak draws."""
    K, i, a = 4096, 33, 2.2
    hist = np.zeros((K, i + 1), dtype=np.int32)
    hist[:, i] = 1
    d = np.concatenate([dp_tables_philox(hist, np.full(K, a), m, 5, r)[0] for m in (0, 5) for r in range(8)])
    e, v = _antoniak_moments(a, i)
    assert abs(d.mean() - e) < 4.5 * math.sqrt(v / d.size) and 0.95 * v < d.var() < 1.05 * v


# gamma + 1 near 1 (d = 2/3, c near 0.41), j = 1 (the same shape regime from the other side), mid shapes, j = 10^6 (c near 3e-4)
@pytest.mark.parametrize("g,j,N", [(1e-3, 1, 200_000), (0.37, 1, 200_000), (1.0, 2, 200_000), (6.5, 40, 100_000),
                                   (1e4, 3, 100_000), (0.37, 5000, 200)])
def test_gamma_doc_terms_distribution(g, j, N):
    from scipy.special import digamma, polygamma
    o = _lengths_oracle(np.full(N, j))
    _, _, eb, ew = o.gamma_doc_stats_philox(0, g, 123, 0, per_entity=True)
    o.close()
    p = j / (j + g)
    assert abs(eb.mean() - p) < 4.5 * math.sqrt(p * (1 - p) / N) + 1e-12
    e = digamma(g + 1) - digamma(g + 1 + j)
    v = polygamma(1, g + 1) - polygamma(1, g + 1 + j)
    assert abs(ew.mean() - e) < 4.5 * math.sqrt(v / N), (ew.mean(), e)
    if N >= 100_000:
        assert 0.96 * v < ew.var() < 1.04 * v, (ew.var(), v)


def test_gamma_doc_terms_at_a_million_tokens():
    """One entity of 10^6 tokens, 600 rounds: Gamma(10^6) with c = 1/sqrt(9d) near 3.3e-4."""
    from scipy.special import digamma, polygamma
    g, j = 1.0, 1_000_000
    o = _lengths_oracle(np.array([j]))
    w = np.array([o.gamma_doc_stats_philox(0, g, 9, r)[1] for r in range(600)])
    o.close()
    e = digamma(g + 1) - digamma(g + 1 + j)
    v = polygamma(1, g + 1) - polygamma(1, g + 1 + j)
    assert abs(w.mean() - e) < 4.5 * math.sqrt(v / len(w)) and 0.7 * v < w.var() < 1.35 * v


# ---------------------------------------------------------------------------- independence of the fields
def test_dp_tables_fields_separate_streams():
    K, L = 512, 60
    hist = np.zeros((K, L), dtype=np.int32)
    hist[:, 40] = 1
    hist[:, 41] = 1
    conc = np.full(K, 3.0)
    base = dp_tables_philox(hist, conc, 0, SEED, 4)[0]
    assert not np.array_equal(base, dp_tables_philox(hist, conc, 7, SEED, 4)[0])            # view
    assert not np.array_equal(base, dp_tables_philox(hist, conc, 0, SEED, 5)[0])            # round
    assert not np.array_equal(base, dp_tables_philox(hist, conc, 0, SEED ^ (1 << 40), 4)[0])  # seed_hi
    # topic: the same cell content in topic t and t+1 is not the same draw
    one = np.zeros((K, L), dtype=np.int32); one[:, 40] = 1
    mk = dp_tables_philox(one, conc, 0, SEED, 4)[0]
    assert len(np.unique(mk)) > 5 and not np.all(mk[1:] == mk[:-1])
    # count: cells i = 40 and i = 41 in a 1e300-free regime draw from different streams (their sum is not 2 x one of them)
    two = np.zeros((K, L), dtype=np.int32); two[:, 41] = 1
    mk2 = dp_tables_philox(two, conc, 0, SEED, 4)[0]
    assert not np.array_equal(mk2, mk) and np.array_equal(mk + mk2, base)


def test_antoniak_fields_separate_streams():
    n = 4096
    items, conc = np.full(n, 80, dtype=np.int32), np.full(n, 4.0)
    a = antoniak_draws_philox(items, conc, SEED, 0)
    assert not np.array_equal(a, antoniak_draws_philox(items, conc, SEED, 1))
    assert not np.array_equal(a, antoniak_draws_philox(items, conc, SEED ^ (1 << 33), 0))
    assert len(np.unique(a)) > 5                                      # draw j: the index separates the streams
    assert np.array_equal(a, antoniak_draws_philox(items, conc, SEED, 0))


def test_gamma_fields_separate_streams_and_sharding_changes_nothing():
    rng = np.random.default_rng(8)
    D = 5000
    lens = rng.integers(1, 30, D)
    o2 = _lengths_oracle([lens, lens], M=2)                           # two views of equal lengths
    _, _, b0, w0 = o2.gamma_doc_stats_philox(0, 1.3, SEED, 7, per_entity=True)
    _, _, b1, w1 = o2.gamma_doc_stats_philox(1, 1.3, SEED, 7, per_entity=True)
    assert np.count_nonzero(w0 == w1) == 0 and np.count_nonzero(b0 != b1) > 0
    _, _, _, wr = o2.gamma_doc_stats_philox(0, 1.3, SEED, 8, per_entity=True)
    assert np.count_nonzero(w0 == wr) == 0
    _, _, _, wh = o2.gamma_doc_stats_philox(0, 1.3, SEED, 7, doc_id_base=2**32, per_entity=True)   # differs only above bit 32
    assert np.count_nonzero(w0 == wh) == 0
    o2.close()
    whole = _lengths_oracle(lens)
    qs, qw, eb, ew = whole.gamma_doc_stats_philox(0, 1.3, SEED, 7, doc_id_base=2**32 + 5, per_entity=True)
    for cuts in ([0, 1700, D], [0, 1, 2999, D], [0, 2500, 2501, 4000, D]):
        sq, sw = 0.0, 0.0
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            sh = _lengths_oracle(lens[lo:hi])
            a, b, sb, sw_e = sh.gamma_doc_stats_philox(0, 1.3, SEED, 7, doc_id_base=2**32 + 5 + lo, per_entity=True)
            sh.close()
            assert np.array_equal(sb, eb[lo:hi]) and np.array_equal(sw_e, ew[lo:hi])
            sq += a; sw += b
        assert sq == qs and math.isclose(sw, qw, rel_tol=1e-12)
    whole.close()
