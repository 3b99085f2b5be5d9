"""Shared pieces of the useVectorsLambda tests: seeded tables, a MixRef beside an oracle or a sampler, state comparisons."""
import numpy as np

from mvtopicmodel_amd.native import Hyper
from mvtopicmodel_amd.synth import Corpus
from tests.helpers import small_corpus
from tests.mix_ref import MixRef


def table(K, V0, seed, rank=3, scale=1.5):
    """expDotProductValues [K][V_0] / sumExpValues [K] from a seeded generator: exp of a low-rank product minus its row maximum (so
    rows are not flat and every entry lies in (0, 1]), the sums those of the table (what one CalcSoftmax call leaves)."""
    rng = np.random.RandomState(seed)
    dot = scale * rng.standard_normal((K, rank)) @ rng.standard_normal((rank, V0))
    e = np.exp(dot - dot.max(axis=1, keepdims=True))
    return e, e.sum(axis=1)


def set_hyper_o(o, hy):
    o.set_hyper(hy.alpha, hy.alpha_sum, hy.beta, hy.beta_sum, hy.gamma, hy.p_a, hy.p_b, hy.inactive)


def make_ref(corpus, hy, z0=None, init_seed=1, cls=MixRef):
    """A MixRef (or, cls=Oracle, the oracle) on the corpus: assignments z0, or the reference's initial draw."""
    o = cls(corpus.K, corpus.V)
    for m in range(corpus.M):
        o.set_corpus(m, corpus.doc_off[m], corpus.tokens[m])
    set_hyper_o(o, hy)
    if z0 is None:
        o.init_assignments(init_seed)
    else:
        for m in range(corpus.M):
            o.set_assignments(m, z0[m])
    o.build_counts()
    return o


def ragged_corpus(K=30, seed=0):
    """two views; entities without view 0, with view 0 only, empty ones; three OOV tokens; a few unassigned ones.  Returns (corpus, z0)."""
    V = [100, 20]
    rng = np.random.RandomState(seed)
    lens0 = np.array([0, 5, 1, 0, 70, 3, 0, 9, 2, 65], dtype=np.int64)
    lens1 = np.array([0, 0, 4, 2, 0, 1, 0, 3, 0, 10], dtype=np.int64)
    off0 = np.concatenate([[0], np.cumsum(lens0)]); off1 = np.concatenate([[0], np.cumsum(lens1)])
    t0 = rng.randint(0, 100, off0[-1]).astype(np.int32); t1 = rng.randint(0, 20, off1[-1]).astype(np.int32)
    t0[[3, 20]] = 100                                           # OOV: type == V (WRK:427-428)
    t1[2] = 25
    c = Corpus(K, V, [off0, off1], [t0, t1])
    z0 = [rng.randint(0, K, off0[-1]).astype(np.int32), rng.randint(0, K, off1[-1]).astype(np.int32)]
    z0[0][[0, 7, 30]] = -1; z0[1][[1, 5]] = -1                  # UNASSIGNED (PTM:63)
    z0[0][[3, 20]] = -1; z0[1][2] = -1                          # (an OOV token is not counted)
    return c, z0


def inactive_case(K=40, V=(300, 50), D=80, lam=(30, 5), seed=51, topics=(33, 36, 39), alpha_new=25.0):
    """a truncated HDP: three inactive topics that hold no token, a likely new-topic branch.  Returns (corpus, hyper, z0)."""
    V = list(V)
    c = small_corpus(K, V, D, list(lam), seed)
    inactive = np.zeros(K, dtype=np.uint8); inactive[list(topics)] = 1
    hy = Hyper.defaults(K, V, inactive=inactive)
    hy.alpha[:, K] = alpha_new
    o = make_ref(c, hy)
    z0 = [o.get_assignments(m) for m in range(c.M)]
    for m in range(c.M):
        z0[m][np.isin(z0[m], list(topics))] = 1
    o.close()
    return c, hy, z0


def same_state(a, b, M, where=""):
    for m in range(M):
        za, zb = a.get_assignments(m), b.get_assignments(m)
        assert np.array_equal(za, zb), f"{where}: z differs in view {m}: {np.count_nonzero(za != zb)} of {len(za)}"
        (wa, ka), (wb, kb) = a.get_counts(m), b.get_counts(m)
        assert np.array_equal(ka, kb), f"{where}: n_k differs in view {m}"
        assert np.array_equal(wa, wb), f"{where}: n_wk differs in view {m}"


STAT_FIELDS = ("tokens", "changed", "new_mass_cnt", "topic_doc_mass_cnt", "word_ftree_mass_cnt", "oov_skipped", "aborted_docs",
               "activated_topic", "activated_modality")


def same_stats(ref_stats, rs, where=""):
    """ref_stats: the dict of a restatement's sweep; rs: another such dict or a sampler's SweepStats"""
    get = (lambda f: rs[f]) if isinstance(rs, dict) else (lambda f: getattr(rs, f))
    for f in STAT_FIELDS:
        assert ref_stats[f] == get(f), f"{where}: {f}: {ref_stats[f]} != {get(f)}"
