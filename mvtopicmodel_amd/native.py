"""NativeSampler — Python mirror of the JNI host class
``org.madgik.MVTopicModel.NativeSampler`` shown in INTEGRATION.md: a thin,
numpy-typed wrapper over the C ABI (include/mvhdp.h).  One instance = one model
shard on one MI355X.  All compute happens in libmvhdp.so on the GPU.
"""
import atexit
import ctypes as C
import sys
import weakref
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np

from ._lib import (CensusRowC, COHORT_BY_COUNT, COHORT_BY_SHARE, CohortArgsC, CohortStatsC, CoocArgsC, CoocStatsC, DIAG_MAX_TOP_WORDS, DIAG_PROPORTIONS, DIAG_ROWS, MAX_M, UNIQUE_ID_BYTES, Config, DebugC, DiagArgsC, DiagOutC,
                   EmbConfigC, EmbStatsC, EntitiesArgsC, EntitiesStatsC, FoldinArgsC, FoldinStatsC, GroupInfoC, HeldoutArgsC, HeldoutStatsC, HyperC, MvhdpError, NearestArgsC, NearestStatsC, PhraseArgsC, PredictArgsC,PhraseStatsC, SimArgsC, SimStatsC, SweepStatsC, TopicGramArgsC, TopicGramStatsC, TuningC,
                   REMAP_RETIRE, RemapArgsC, RemapStatsC, SPLIT_KEEP_ALPHA, SplitArgsC, SplitStatsC,
                   load_library,
                   SIM_COS, SIM_COS_FOLDED, SIM_JSD)

SWEEP_REUSE_TREES = 0x1
SWEEP_NO_APPLY = 0x2
SWEEP_EXACT_CHAIN = 0x4
SWEEP_GENERIC_KERNEL = 0x8
SWEEP_FROZEN = 0x10
SWEEP_LIVE = 0x20
SWEEP_SEGMENT_APPLY = 0x40
SWEEP_SEGMENT_OVERLAP = 0x80
SWEEP_ASYNC_EXCHANGE = 0x100
SWEEP_SHARD_BIRTHS = 0x200


def SWEEP_LIVE_SEGMENTS(n):
    return (int(n) & 0xFF) << 16

def SWEEP_ONLY_SEGMENT(s):
    return ((int(s) + 1) & 0xFF) << 24


EMB_SERIAL = 0x1

BUF_COUNTS = 0
BUF_DELTA = 1
BUF_BIRTH_KEYS = 2
BUF_COUNTS12 = 3        # read-only views for tests and diagnostics: the 12-bit image of n_wk and the row classes
BUF_ROW_CLASS = 4
ACT_KEY_NONE = (1 << 63) - 1

# a row of the launch census (NativeSampler.sweep_census): key = (rmax, debug, walk, narrow, roomy, liverows, mix)
CensusRow = namedtuple("CensusRow", "key launches tokens")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_live = weakref.WeakSet()          # open samplers, closed at exit while the HIP runtime is still alive


@atexit.register
def _close_all():
    for s in list(_live):
        try:
            s.close()
        except Exception:
            pass


@dataclass
class Hyper:
    """The hyper-parameters the sampler reads (PTM:79-83,95,130-131)."""
    alpha: np.ndarray          # [M][K+1]
    alpha_sum: np.ndarray      # [M]
    beta: np.ndarray           # [M]
    beta_sum: np.ndarray       # [M]
    gamma: np.ndarray          # [M]
    p_a: np.ndarray            # [M][M]
    p_b: np.ndarray            # [M][M]
    inactive: np.ndarray = None  # [K] uint8 or None

    @staticmethod
    def defaults(K, V, alpha=0.1, beta=0.01, p_a=0.31, p_b=1.0, inactive=None):
        """PTM:207-214 (alpha[m][.]=alpha, alphaSum=K*alpha, gamma=1, beta) + betaSum=beta*V_m PTM:420.
        p_a = 0.31 is iteration 1 of the burn-in schedule PTM:1168."""
        M = len(V)
        return Hyper(alpha=np.full((M, K + 1), alpha, dtype=np.float64),
                     alpha_sum=np.full(M, K * alpha, dtype=np.float64),
                     beta=np.full(M, beta, dtype=np.float64),
                     beta_sum=np.array([beta * v for v in V], dtype=np.float64),
                     gamma=np.ones(M, dtype=np.float64),
                     p_a=np.full((M, M), p_a, dtype=np.float64),
                     p_b=np.full((M, M), p_b, dtype=np.float64),
                     inactive=None if inactive is None else np.asarray(inactive, dtype=np.uint8))


@dataclass
class SweepStats:
    tokens: int = 0
    changed: int = 0
    new_mass_cnt: int = 0
    topic_doc_mass_cnt: int = 0
    word_ftree_mass_cnt: int = 0
    oov_skipped: int = 0
    aborted_docs: int = 0
    exact_fallbacks: int = 0
    activated_topic: int = -1
    activated_modality: int = -1
    activation_key: int = 0
    sweep_kernel_ms: float = 0.0
    total_ms: float = 0.0
    activations: int = 0
    reserved: int = 0
    dbg: list = field(default=None, repr=False)
    trace: np.ndarray = field(default=None, repr=False)


@dataclass
class SimStats:
    """mvhdp_sim_stats: what a similar_pairs call did.  pairs_screened: matrix cells of the first stage (128 x 128 per launched tile)."""
    pairs_screened: int = 0
    candidates: int = 0
    emitted: int = 0
    stripes: int = 0
    regrown: int = 0
    margin: float = 0.0


SIM_METRICS = {"cos_folded": SIM_COS_FOLDED, "cos": SIM_COS, "jsd": SIM_JSD}


def _sim_stats(c):
    return SimStats(**{f: getattr(c, f) for f, _ in SimStatsC._fields_})


def sim_probe(n, dim, stripe_rows=0):
    """mvhdp_sim_probe: margin, stripes and pairs_screened of a cosine similar_pairs call of that shape.  No device."""
    st = SimStatsC()
    rc = load_library().mvhdp_sim_probe(int(n), int(dim), int(stripe_rows), C.byref(st))
    if rc != 0:
        raise MvhdpError(rc, "sim_probe: bad shape" if rc == -1 else "sim_probe: dim > 65536")
    return _sim_stats(st)


@dataclass
class NearestStats:
    """mvhdp_nearest_stats: what a nearest_entities call did.  cells_screened: matrix cells of the first stage (128 x 128 per launched
    tile); candidates: pairs the exact stage recomputed; exact_only_rows: query and candidate rows that were not screened."""
    cells_screened: int = 0
    candidates: int = 0
    exact_only_rows: int = 0
    blocks: int = 0
    regrown: int = 0
    margin: float = 0.0


@dataclass
class NearestResult:
    """mvhdp_nearest_entities: per query row its first counts[q] entities by (sim descending, entity id ascending): ids [nq][n] (-1
    unfilled), sims [nq][n] (0.0 unfilled), counts [nq]."""
    ids: np.ndarray
    sims: np.ndarray
    counts: np.ndarray
    stats: NearestStats = None


def _nearest_stats(c):
    return NearestStats(**{f: getattr(c, f) for f, _ in NearestStatsC._fields_})


def nearest_probe(nq, nc, K, block_queries=0, stripe_candidates=0):
    """mvhdp_nearest_probe: margin, blocks and cells_screened of a nearest_entities call of that shape.  No device."""
    st = NearestStatsC()
    rc = load_library().mvhdp_nearest_probe(int(nq), int(nc), int(K), int(block_queries), int(stripe_candidates), C.byref(st))
    if rc != 0:
        raise MvhdpError(rc, "nearest_probe: bad shape" if rc == -1 else "nearest_probe: K > 65536")
    return _nearest_stats(st)


def _first_n(values, ids, n):
    """positions of the first n of (value descending, id ascending); NaN values left out"""
    keep = np.flatnonzero(~np.isnan(values))
    order = keep[np.lexsort((ids[keep], -values[keep]))]
    return order[:n]


def merge_nearest(results, n):
    """The NearestResult over the union of the candidate ranges from the results of its parts (document shards, or pieces of one
    range), ids already in one numbering: per query the first n of all listed entries by the same order.  A value belongs to its pair
    alone, so the merge is exact provided every part was asked for at least n.  No device."""
    results = list(results)
    n = int(n)
    nq = len(results[0].counts)
    if any(len(r.counts) != nq for r in results):
        raise ValueError("merge_nearest: the results disagree on the number of queries")
    ids = np.full((nq, n), -1, dtype=np.int64)
    sims = np.zeros((nq, n), dtype=np.float64)
    counts = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        i = np.concatenate([r.ids[q, :r.counts[q]] for r in results])
        v = np.concatenate([r.sims[q, :r.counts[q]] for r in results])
        o = _first_n(v, i, n)
        counts[q] = len(o)
        ids[q, :len(o)], sims[q, :len(o)] = i[o], v[o]
    st = [r.stats for r in results if r.stats is not None]
    stats = NearestStats(sum(x.cells_screened for x in st), sum(x.candidates for x in st), sum(x.exact_only_rows for x in st),
                         sum(x.blocks for x in st), sum(x.regrown for x in st), max(x.margin for x in st)) if st else None
    return NearestResult(ids, sims, counts, stats)


@dataclass
class EntitiesStats:
    """mvhdp_entities_stats: cells = scores computed, excluded = (entity, query) cells marked, blocks = blocks of scores, kernel_ms = the
    stream's time from the first kernel to the last."""
    cells: int = 0
    excluded: int = 0
    blocks: int = 0
    kernel_ms: float = 0.0


@dataclass
class EntityRanking:
    """mvhdp_predict_entities: per query its first counts[j] candidate entities by (score descending, entity id ascending): ids [nq][n]
    (-1 unfilled), scores [nq][n] (0.0 unfilled), counts [nq]."""
    ids: np.ndarray
    scores: np.ndarray
    counts: np.ndarray
    stats: EntitiesStats = None


@dataclass
class EntityRanks:
    """mvhdp_rank_entities: per (query, entity) pair its score and the number of candidates that are not excluded and precede it."""
    score: np.ndarray
    rank: np.ndarray

    def recall_at(self, n):
        return float(np.mean(self.rank < n)) if len(self.rank) else float("nan")

    def mrr(self):
        return float(np.mean(1.0 / (self.rank + 1.0))) if len(self.rank) else float("nan")


def merge_predicted_entities(results, n):
    """The EntityRanking over the union of the candidate ranges from the results of its parts (document shards, or pieces of one range),
    ids already in one numbering: per query the first n of all listed entries by (score descending, id ascending).  A score belongs to
    its (entity, query) alone, so the merge is exact provided every part was asked for at least n.  No device."""
    results = list(results)
    n = int(n)
    nq = len(results[0].counts)
    if any(len(r.counts) != nq for r in results):
        raise ValueError("merge_predicted_entities: the results disagree on the number of queries")
    ids = np.full((nq, n), -1, dtype=np.int64)
    scores = np.zeros((nq, n), dtype=np.float64)
    counts = np.zeros(nq, dtype=np.int32)
    for q in range(nq):
        i = np.concatenate([r.ids[q, :r.counts[q]] for r in results])
        v = np.concatenate([r.scores[q, :r.counts[q]] for r in results])
        o = _first_n(v, i, n)
        counts[q] = len(o)
        ids[q, :len(o)], scores[q, :len(o)] = i[o], v[o]
    st = [r.stats for r in results if r.stats is not None]
    stats = EntitiesStats(sum(x.cells for x in st), sum(x.excluded for x in st), sum(x.blocks for x in st), sum(x.kernel_ms for x in st)) if st else None
    return EntityRanking(ids, scores, counts, stats)


@dataclass
class TopicGramStats:
    """mvhdp_topic_gram_stats: rows = r1 - r0, blocks = blocks of MVHDP_GRAM_BLOCK_ROWS rows, passes = passes of blocks_per_pass blocks,
    kernel_ms = the stream's time from the first kernel to the last."""
    rows: int = 0
    blocks: int = 0
    passes: int = 0
    kernel_ms: float = 0.0


@dataclass
class TopicGram:
    """mvhdp_topic_gram: gram [K][K] = sum_r y_r[k] y_r[l] and sums [K] = sum_r y_r[k] in the contract's fixed order (y = X or sqrt(X) by
    `transform`), n_above [K] and co_above [K][K] the exact counts of rows with X > threshold (None when no threshold was given), rows =
    the number of rows.  The methods below are HOST derivations by numpy: convenient, not pinned to bits."""
    gram: np.ndarray
    sums: np.ndarray
    n_above: np.ndarray
    co_above: np.ndarray
    rows: int
    transform: str
    stats: TopicGramStats = None

    def _need(self, transform, what):
        if self.transform != transform:
            raise ValueError(f"{what} needs transform={transform!r}")

    def _need_counts(self, what):
        if self.n_above is None or self.co_above is None:
            raise ValueError(f"{what} needs a threshold")

    def cosine(self):
        """gram[k][l] / sqrt(gram[k][k] gram[l][l]) (identity transform); NaN where a column is all zero.  A host derivation, not pinned
        to bits."""
        self._need("identity", "cosine")
        d = np.sqrt(np.diag(self.gram))
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.gram / np.outer(d, d)

    def correlation(self):
        """Pearson correlation of two columns across the rows, from gram, sums and rows (identity transform); NaN for a constant column.
        A host derivation, not pinned to bits."""
        self._need("identity", "correlation")
        n = float(self.rows)
        with np.errstate(divide="ignore", invalid="ignore"):
            cov = self.gram / n - np.outer(self.sums, self.sums) / (n * n)
            d = np.sqrt(np.diag(cov))
            return cov / np.outer(d, d)

    def bhattacharyya(self):
        """sum_r sqrt(X_r[k] X_r[l]) = the gram of the sqrt transform, each cell divided by sqrt(S_k S_l), S_k = gram[k][k] = the column's
        sum of X: columns that are distributions (phi over a whole view) have S_k = 1 up to rounding.  A host derivation, not pinned to bits."""
        self._need("sqrt", "bhattacharyya")
        d = np.sqrt(np.diag(self.gram))
        with np.errstate(divide="ignore", invalid="ignore"):
            return self.gram / np.outer(d, d)

    def hellinger(self):
        """sqrt(1 - bhattacharyya()), clipped at 0.  A host derivation, not pinned to bits."""
        return np.sqrt(np.clip(1.0 - self.bhattacharyya(), 0.0, None))

    def jaccard(self):
        """co_above / (n_above[k] + n_above[l] - co_above); NaN where neither column has a row above.  A host derivation."""
        self._need_counts("jaccard")
        co = self.co_above.astype(np.float64)
        n = self.n_above.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return co / (n[:, None] + n[None, :] - co)

    def npmi(self):
        """Normalised pointwise mutual information of 'above the threshold' across the rows: log(p_kl / (p_k p_l)) / -log(p_kl); -1 where
        two topics never meet, NaN where a topic has no row above.  A host derivation, not pinned to bits."""
        self._need_counts("npmi")
        n = float(self.rows)
        with np.errstate(divide="ignore", invalid="ignore"):
            pkl = self.co_above / n
            pk = self.n_above / n
            out = np.log(pkl / np.outer(pk, pk)) / -np.log(pkl)
            out[(self.co_above == 0) & (np.outer(self.n_above, self.n_above) > 0)] = -1.0
        return out


def merge_topic_grams(parts):
    """The TopicGram over the union of the rows of its parts (document shards, or pieces of one range): the integers are added exactly;
    gram and sums are added in list order, cell by cell in fp64 -- the list-order sum of the parts' results, not the bits a single call
    over all the rows would give.  No device."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_topic_grams: no parts")
    if any(p.transform != parts[0].transform or p.gram.shape != parts[0].gram.shape for p in parts):
        raise ValueError("merge_topic_grams: the parts disagree on the transform or on K")
    if any((p.n_above is None) != (parts[0].n_above is None) for p in parts):
        raise ValueError("merge_topic_grams: some parts have counts and some do not")
    gram = np.zeros_like(parts[0].gram)
    sums = np.zeros_like(parts[0].sums)
    for p in parts:
        gram = gram + p.gram
        sums = sums + p.sums
    n_above = co_above = None
    if parts[0].n_above is not None:
        n_above = np.sum([p.n_above for p in parts], axis=0, dtype=np.int64)
        co_above = np.sum([p.co_above for p in parts], axis=0, dtype=np.int64)
    st = [p.stats for p in parts if p.stats is not None]
    stats = TopicGramStats(sum(x.rows for x in st), sum(x.blocks for x in st), sum(x.passes for x in st), sum(x.kernel_ms for x in st)) if st else None
    return TopicGram(gram, sums, n_above, co_above, sum(int(p.rows) for p in parts), parts[0].transform, stats)


def _member_csr(groups):
    """(member_off [G+1], members) as int64 from a list of entity-id lists, or from the pair itself"""
    if isinstance(groups, tuple):
        moff = np.ascontiguousarray(groups[0], dtype=np.int64)
        mem = np.ascontiguousarray(groups[1], dtype=np.int64)
    else:
        moff = np.zeros(len(groups) + 1, dtype=np.int64)
        moff[1:] = np.cumsum([len(g) for g in groups])
        mem = np.ascontiguousarray(np.concatenate([np.asarray(g, dtype=np.int64) for g in groups]) if len(groups) else [], dtype=np.int64)
    if moff.ndim != 1 or len(moff) < 1 or len(mem) != int(moff[-1]):
        raise ValueError("member_off / members shape mismatch")
    return moff, mem


@dataclass
class CohortStats:
    """mvhdp_cohort_stats: listings = member_off[n_cohorts], tokens = the counted tokens over all listings, skipped = the skipped ones
    (z == -1 or out of the vocabulary), once per listing; passes of cohorts_per_pass cohorts; kernel_ms = the stream's time from the
    first kernel to the last."""
    listings: int = 0
    tokens: int = 0
    skipped: int = 0
    passes: int = 0
    cohorts_per_pass: int = 0
    kernel_ms: float = 0.0


@dataclass
class CohortWords:
    """mvhdp_cohort_top_words: per cohort g and topic k the top types [G][K][n] (-1 unfilled) with their counts inside the cohort
    [G][K][n], nonzero [G][K] = the types with a count, tokens [G][K] = the cohort's tokens of the topic, docs [G][K] = the listings that
    hold the topic.  types, counts and nonzero are None for a trends-only call."""
    types: np.ndarray
    counts: np.ndarray
    nonzero: np.ndarray
    tokens: np.ndarray
    docs: np.ndarray
    stats: CohortStats = None

    def trend(self):
        """tokens normalised per cohort: [G][K] rows that sum to 1 (a row of zeros for a cohort without counted tokens).
        A host derivation by numpy, not pinned to bits."""
        t = self.tokens.astype(np.float64)
        tot = t.sum(axis=1, keepdims=True)
        return np.divide(t, tot, out=np.zeros_like(t), where=tot > 0)

    def words(self, g, k, vocabulary=None):
        """The list of cohort g and topic k as [(type id or vocabulary[type], count)], the unfilled slots dropped.  A host derivation."""
        if self.types is None:
            raise ValueError("words needs a call that was not trends-only")
        return [(int(t) if vocabulary is None else vocabulary[int(t)], int(c)) for t, c in zip(self.types[g, k], self.counts[g, k]) if t >= 0]


@dataclass
class CoocStats:
    """mvhdp_cooc_stats: entities = the non-empty spans read, tokens = the positions read, hits = the positions whose type sits in at least
    one set, oov = the positions with a type outside the vocabulary, distinct_words = the distinct types over all sets, memberships = the
    filled slots; kernel_ms = the stream's time from the first kernel to the last."""
    entities: int = 0
    tokens: int = 0
    hits: int = 0
    oov: int = 0
    distinct_words: int = 0
    memberships: int = 0
    kernel_ms: float = 0.0


COOC_MEASURES = ("uci", "npmi", "umass")


@dataclass
class WordCooccurrence:
    """mvhdp_word_cooccurrence: co [S][n][n] (int64) = the windows in which the slots i and j of set s are both present (the diagonal: in
    which slot i is present), windows = the windows of the entity range, sets [S][n] = the word sets as they were passed (-1 = empty slot).
    The measures below are host derivations by numpy from these integers.  Their formulas are ours and are stated in full; they are the
    usual definitions of the literature, but no equality with any toolkit's numbers is claimed."""
    co: np.ndarray
    windows: int
    sets: np.ndarray
    stats: CoocStats = None

    def occurrences(self):
        """[S][n]: the windows in which each slot is present (the diagonals of co).  A host derivation."""
        return np.diagonal(self.co, axis1=1, axis2=2).copy()

    def pair_scores(self, measure, eps=1e-12):
        """[S][n][n] float64, a host derivation.  With p_i = co_ii / windows and p_ij = co_ij / windows:
          "uci":   log((p_ij + eps) / (p_i p_j))
          "npmi":  the same divided by -log(p_ij + eps)
          "umass": for j < i in slot order log((p_ij + eps) / p_j); the upper triangle and the diagonal are NaN
        A pair with an empty slot, or with co_ii == 0 or co_jj == 0, is NaN."""
        if measure not in COOC_MEASURES:
            raise ValueError('measure must be "uci", "npmi" or "umass"')
        occ = self.occurrences()
        ok = (np.asarray(self.sets) >= 0) & (occ > 0)
        defined = ok[:, :, None] & ok[:, None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            p = occ.astype(np.float64) / float(self.windows) if self.windows > 0 else np.full(occ.shape, np.nan)
            pij = self.co.astype(np.float64) / float(self.windows) if self.windows > 0 else np.full(self.co.shape, np.nan)
            if measure == "umass":
                out = np.log((pij + eps) / p[:, None, :])
                n = out.shape[1]
                defined = defined & np.tril(np.ones((n, n), dtype=bool), -1)[None]
            else:
                out = np.log((pij + eps) / (p[:, :, None] * p[:, None, :]))
                if measure == "npmi":
                    out = out / -np.log(pij + eps)
        return np.where(defined, out, np.nan)

    def coherence(self, measure, aggregate="mean", eps=1e-12):
        """[S] float64: per set the mean (or "sum") of pair_scores over the pairs j < i, NaN pairs skipped; NaN for a set without a
        defined pair.  A host derivation."""
        if aggregate not in ("mean", "sum"):
            raise ValueError('aggregate must be "mean" or "sum"')
        sc = self.pair_scores(measure, eps)
        n = sc.shape[1]
        low = np.tril(np.ones((n, n), dtype=bool), -1)[None]
        use = low & ~np.isnan(sc)
        cnt = use.sum(axis=(1, 2))
        tot = np.where(use, sc, 0.0).sum(axis=(1, 2))
        with np.errstate(divide="ignore", invalid="ignore"):
            val = tot / cnt if aggregate == "mean" else tot
        return np.where(cnt > 0, val, np.nan)


def _word_sets(sets):
    """[S][n] int32 from an int array or from a list of lists, the short rows padded with -1"""
    if isinstance(sets, np.ndarray):
        out = np.ascontiguousarray(sets, dtype=np.int32)
    else:
        rows = [list(r) for r in sets]
        n = max([len(r) for r in rows], default=0)
        out = np.full((len(rows), n), -1, dtype=np.int32)
        for i, r in enumerate(rows):
            out[i, :len(r)] = r
    if out.ndim != 2:
        raise ValueError("sets must be [S][n]")
    return out


def merge_word_cooccurrence(parts):
    """The WordCooccurrence of a corpus from those of disjoint entity ranges (or document shards) over the same sets: co, windows and the
    additive stats summed -- exact, because a window never crosses an entity.  Refuses parts whose sets differ.  No device."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_word_cooccurrence: no parts")
    for p in parts[1:]:
        if p.sets.shape != parts[0].sets.shape or not np.array_equal(p.sets, parts[0].sets):
            raise ValueError("merge_word_cooccurrence: the parts were counted for different sets")
    st = [p.stats for p in parts if p.stats is not None]
    stats = CoocStats(sum(s.entities for s in st), sum(s.tokens for s in st), sum(s.hits for s in st), sum(s.oov for s in st),
                      st[0].distinct_words if st else 0, st[0].memberships if st else 0, sum(s.kernel_ms for s in st))
    return WordCooccurrence(np.sum([p.co for p in parts], axis=0, dtype=np.int64), sum(int(p.windows) for p in parts), parts[0].sets.copy(), stats)


@dataclass
class RemapStats:
    """mvhdp_remap_stats: per view the tokens whose topic changed to another topic (moved [M]) and those that became unassigned (dropped
    [M]); vacated = the topics no topic maps onto that held tokens or were active before, retired = those of them that are inactive
    afterwards; kernel_ms = the stream's time over both passes."""
    moved: np.ndarray = None
    dropped: np.ndarray = None
    vacated: int = 0
    retired: int = 0
    kernel_ms: float = 0.0


def _remap_call(fn, handle, K, M, topic_map, retire):
    """the arguments and the statistics of mvhdp_remap_topics / mvhdp_group_remap_topics; returns (rc, RemapStats)"""
    tm = np.ascontiguousarray(topic_map, dtype=np.int32)
    if tm.shape != (K,):
        raise ValueError(f"remap_topics: the map must hold one entry per topic ({K}), got shape {tm.shape}")
    a = RemapArgsC(tm.ctypes.data, REMAP_RETIRE if retire else 0)
    st = RemapStatsC()
    rc = fn(handle, C.byref(a), C.byref(st))
    return rc, RemapStats(np.array(st.moved[:M], dtype=np.int64), np.array(st.dropped[:M], dtype=np.int64), st.vacated, st.retired, st.kernel_ms)


@dataclass
class SplitStats:
    """mvhdp_split_stats: per view the tokens that carried the source topic (split [M]) and those of them in the target at the end (moved
    [M]); flips [iterations] = the tokens that changed side per iteration, flips_last its last entry (0 without iterations); target = the
    index used, activated = whether it left the inactive set; kernel_ms = the stream's time over the kernels of the call."""
    split: np.ndarray = None
    moved: np.ndarray = None
    flips_last: int = 0
    target: int = -1
    activated: bool = False
    kernel_ms: float = 0.0
    flips: np.ndarray = None


def merge_topic_top_entities(parts, n):
    """(ids [K][n], weights [K][n], counts [K]) over the union of the entity ranges from the same triples of its parts, ids in one
    numbering: per topic the first n by (weight descending, id ascending).  Exact, as merge_nearest is.  No device."""
    parts = list(parts)
    n = int(n)
    K = len(parts[0][2])
    ids = np.full((K, n), -1, dtype=np.int64)
    weights = np.zeros((K, n), dtype=np.float64)
    counts = np.zeros(K, dtype=np.int32)
    for k in range(K):
        i = np.concatenate([p[0][k, :p[2][k]] for p in parts])
        v = np.concatenate([p[1][k, :p[2][k]] for p in parts])
        o = _first_n(v, i, n)
        counts[k] = len(o)
        ids[k, :len(o)], weights[k, :len(o)] = i[o], v[o]
    return ids, weights, counts


@dataclass
class PhraseStats:
    """mvhdp_phrase_stats: maximal same-topic runs, phrase occurrences, distinct phrases, phrases kept, and the comparisons in which the
    used hash bits were equal and the phrases were not."""
    runs: int = 0
    occurrences: int = 0
    distinct: int = 0
    kept: int = 0
    hash_collisions: int = 0


@dataclass
class TopicPhrases:
    """findTopicPhrases PTM:1921-1976 per topic: phrases[k] = [(key, count), ...] by count descending, equal counts by word-id sequence
    ascending (a proper prefix first), cut at max_per_topic; key = the word-id tuple, or the words joined by a blank when a vocabulary was
    given.  distinct[k] / occurrences[k]: the topic's phrases and the sum of their counts BEFORE the cut (count / occurrences[k] is the
    phrase weight of PTM:2037)."""
    phrases: list
    distinct: np.ndarray
    occurrences: np.ndarray
    stats: PhraseStats = None


def _phrase_order(table, max_per_topic):
    """[(ids, count)] in the order of include/mvhdp.h, cut"""
    out = sorted(table, key=lambda e: (-e[1], e[0]))
    return out if max_per_topic < 0 else out[:max_per_topic]


def merge_topic_phrases(results, max_per_topic):
    """The TopicPhrases of a corpus from the UNCUT ones (max_per_topic < 0, no vocabulary) of its document shards: equal keys summed, the
    same order, the same cut.  Phrases never cross an entity, so for document shards this is exact.  No device."""
    results = list(results)
    K = len(results[0].phrases)
    merged = []
    for k in range(K):
        acc = {}
        for r in results:
            if len(r.phrases) != K:
                raise ValueError("merge_topic_phrases: the results disagree on the number of topics")
            for ids, c in r.phrases[k]:
                if not isinstance(ids, tuple):
                    raise ValueError("merge_topic_phrases: results with a vocabulary cannot be merged (ask for word-id tuples)")
                acc[ids] = acc.get(ids, 0) + int(c)
        merged.append(acc)
    for r in results:
        if any(len(r.phrases[k]) != int(r.distinct[k]) for k in range(K)):
            raise ValueError("merge_topic_phrases: a result was cut (max_per_topic must be < 0 on the shards)")
    distinct = np.array([len(a) for a in merged], dtype=np.int64)
    occurrences = np.sum([np.asarray(r.occurrences, dtype=np.int64) for r in results], axis=0).astype(np.int64)
    phrases = [_phrase_order(list(a.items()), int(max_per_topic)) for a in merged]
    st = PhraseStats(runs=sum(r.stats.runs for r in results if r.stats), occurrences=int(occurrences.sum()), distinct=int(distinct.sum()),
                     kept=sum(len(p) for p in phrases), hash_collisions=sum(r.stats.hash_collisions for r in results if r.stats))
    return TopicPhrases(phrases, distinct, occurrences, st)


@dataclass
class HeldoutResult:
    """mvhdp_heldout_left_to_right: the left-to-right estimate of log p(held-out documents | model).  doc_log_likelihood [D];
    position_sum [N] = S[n], the particles' p(w_n | w_<n) added up (0 at an out-of-vocabulary position), or None; doc_tokens [D] and
    tokens count the in-vocabulary tokens; visits = weight vectors formed over all particles."""
    log_likelihood: float
    doc_log_likelihood: np.ndarray
    position_sum: np.ndarray
    doc_tokens: np.ndarray
    tokens: int = 0
    oov: int = 0
    visits: int = 0
    particles: int = 0

    @property
    def perplexity(self):
        return float(np.exp(-self.log_likelihood / self.tokens)) if self.tokens else float("nan")


@dataclass
class FoldinResult:
    """mvhdp_fold_in: theta [D][K], the topic proportions of the folded-in documents (None without view_weights); z, a list of M arrays
    (-1: out of vocabulary or unassigned; None for a view no document has) or None; counts_sum [D][M][K], n_dk added over the recorded
    states, or None; tokens (in vocabulary) and oov over all views; visits = weight vectors formed; kernel_ms = the kernel's time."""
    theta: np.ndarray
    z: list
    counts_sum: np.ndarray
    tokens: int = 0
    oov: int = 0
    visits: int = 0
    kernel_ms: float = 0.0


@dataclass
class ItemScores:
    """mvhdp_score_items: per queried (entity, item) pair the model's score and the item's 0-based rank among the view's types that are
    not excluded for the entity (include/mvhdp.h).  The summaries are the host's arithmetic on those two arrays."""
    score: np.ndarray
    rank: np.ndarray

    def mean_log_score(self):
        """mean over the pairs of log score (-inf if a score is 0; nan without pairs)"""
        if len(self.score) == 0:
            return float("nan")
        with np.errstate(divide="ignore"):
            return float(np.mean(np.log(self.score)))

    def recall_at(self, n):
        """the share of the pairs whose item is among the entity's first n"""
        return float(np.mean(self.rank < int(n))) if len(self.rank) else float("nan")

    def mrr(self):
        """mean reciprocal rank, 1 / (rank + 1)"""
        return float(np.mean(1.0 / (self.rank.astype(np.float64) + 1.0))) if len(self.rank) else float("nan")


def _heldout_docs(doc_off, tokens):
    doc_off = np.ascontiguousarray(doc_off, dtype=np.int64)
    tokens = np.ascontiguousarray(tokens, dtype=np.int32)
    if doc_off.ndim != 1 or len(doc_off) < 1 or len(tokens) != int(doc_off[-1]):
        raise ValueError("doc_off/tokens shape mismatch")
    return doc_off, tokens


def round_similarity(sim):
    """The flow's (double) Math.round(similarity * 1000) / 1000 (FLOW:1152,1467,1488) for the non-negative values it stores."""
    return np.floor(np.asarray(sim, dtype=np.float64) * 1000 + 0.5) / 1000


@dataclass
class EmbConfig:
    """mvhdp_emb_config: the shape of TopicWordEmbeddings(alphabet[0], C, Cc, window, K, ..) (TWE:126-163) and what countWords /
    train take.  defaults() are the reference's values: C = vectorSize 200 (FLOW:74), Cc = 50 (PTM:523), train(data, threads, 5, 2)."""
    num_columns: int = 200
    num_context_columns: int = 50
    with_topics: bool = True
    window: int = 5
    num_samples: int = 5
    min_doc_length: int = 10
    sampling_table_size: int = 100_000_000
    sampling_factor: float = 1e-4
    min_exp: float = -6.0
    max_exp: float = 6.0
    sigmoid_cache_size: int = 1000

    @staticmethod
    def defaults(with_topics=True, **kw):
        kw.setdefault("num_context_columns", 50 if with_topics else 0)
        return EmbConfig(with_topics=bool(with_topics), **kw)

    def to_c(self):
        return EmbConfigC(int(self.num_columns), int(self.num_context_columns), int(bool(self.with_topics)), int(self.window),
                          int(self.num_samples), int(self.min_doc_length), int(self.sampling_table_size), float(self.sampling_factor),
                          float(self.min_exp), float(self.max_exp), int(self.sigmoid_cache_size), 0)


@dataclass
class EmbStats:
    words_so_far: int = 0
    words_sampled: int = 0
    words_considered: int = 0
    docs_skipped: int = 0
    calls: int = 0
    negatives_skipped: int = 0
    residual: float = 0.0
    last_epoch_residual: float = 0.0
    last_epoch_calls: int = 0
    kernel_ms: float = 0.0


def java_string_lengths(vocabulary):
    """String.length() of every word: UTF-16 code units (a character outside the BMP counts twice)."""
    return np.array([len(str(w).encode("utf-16-le")) // 2 for w in vocabulary], dtype=np.int32)


@dataclass
class Diagnostics:
    """What mvhdp_diagnostics returns (FastQMVWVTopicModelDiagnostics, DIAG:53-236): the thirteen score rows by name (DIAG:104-116),
    the topic-word scores of the same rows ([K][N]; zero for the rows that define none), the co-document matrices and the
    accumulators of collectDocumentStatistics, the view-0 top words and discrWeightPerModality (PTM:2181-2230)."""
    scores: dict
    word_scores: dict
    codoc: np.ndarray                   # [K][N][N]
    top_words: np.ndarray               # [K][N] view-0 type ids, -1 where a topic has fewer than N words
    top_counts: np.ndarray              # [K][N]
    nonzero: np.ndarray                 # [K] words with n_wk > 0
    num_rank1_docs: np.ndarray          # [K]
    num_nonzero_docs: np.ndarray        # [K]
    num_docs_at_proportions: np.ndarray  # [K][7]
    sum_count_log_count: np.ndarray     # [K]
    word_type_counts: np.ndarray        # [V_0]
    num_tokens: int
    discr_weight_per_view: np.ndarray   # [M]


def _run_diagnostics(L, fn, handle, K, V0, M, num_top_words, vocabulary, word_length):
    N = int(num_top_words)
    if word_length is None and vocabulary is not None:
        if len(vocabulary) != V0:
            raise ValueError(f"vocabulary has {len(vocabulary)} words, view 0 has {V0} types")
        word_length = java_string_lengths(vocabulary)
    wl = None if word_length is None else np.ascontiguousarray(word_length, dtype=np.int32)
    if wl is not None and wl.shape != (V0,):
        raise ValueError("word_length must be [V_0]")
    nn = max(N, 1)
    R = len(DIAG_ROWS)
    a = dict(scores=np.zeros((R, K)), word_scores=np.zeros((R, K, nn)), codoc=np.zeros((K, nn, nn), np.int32),
             top_types=np.zeros((K, nn), np.int32), top_counts=np.zeros((K, nn), np.int32), nonzero=np.zeros(K, np.int32),
             num_rank1_docs=np.zeros(K, np.int32), num_nonzero_docs=np.zeros(K, np.int32),
             num_docs_at_proportions=np.zeros((K, DIAG_PROPORTIONS), np.int32), sum_count_log_count=np.zeros(K),
             word_type_counts=np.zeros(V0, np.int32), num_tokens=np.zeros(1, np.int64), discr_weight_per_view=np.zeros(M))
    args = DiagArgsC(N, None if wl is None else wl.ctypes.data)
    out = DiagOutC(**{f: a[f].ctypes.data for f, _ in DiagOutC._fields_})
    rc = fn(handle, C.byref(args), C.byref(out))
    if rc != 0:
        return rc, None
    return 0, Diagnostics(scores={n: a["scores"][i] for i, n in enumerate(DIAG_ROWS)},
                          word_scores={n: a["word_scores"][i] for i, n in enumerate(DIAG_ROWS)},
                          codoc=a["codoc"], top_words=a["top_types"], top_counts=a["top_counts"], nonzero=a["nonzero"],
                          num_rank1_docs=a["num_rank1_docs"], num_nonzero_docs=a["num_nonzero_docs"],
                          num_docs_at_proportions=a["num_docs_at_proportions"], sum_count_log_count=a["sum_count_log_count"],
                          word_type_counts=a["word_type_counts"], num_tokens=int(a["num_tokens"][0]),
                          discr_weight_per_view=a["discr_weight_per_view"])


class NativeSampler:
    def __init__(self, K, V, device=0, doc_id_base=0):
        self.L = load_library()
        self.K = int(K)
        self.V = [int(v) for v in V]
        self.M = len(self.V)
        if self.M > MAX_M:
            raise ValueError("too many modalities")
        cfg = Config()
        cfg.num_topics = self.K
        cfg.num_modalities = self.M
        for m, v in enumerate(self.V):
            cfg.num_types[m] = v
        cfg.device = int(device)
        cfg.doc_id_base = int(doc_id_base)
        self.h = C.c_void_p()
        rc = self.L.mvhdp_create(C.byref(cfg), C.byref(self.h))
        _live.add(self)
        if rc != 0:
            msg = self.L.mvhdp_last_error(None).decode()
            self.h = None
            raise MvhdpError(rc, msg)
        self.N = [0] * self.M
        self.D = 0

    # -- lifetime ---------------------------------------------------------
    def close(self):
        if getattr(self, "h", None):
            self.L.mvhdp_destroy(self.h)
            self.h = None

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be gone: handles still open then were closed by
        # the atexit hook below, while the runtime was alive
        if sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, rc):
        if rc != 0:
            raise MvhdpError(rc, self.L.mvhdp_last_error(self.h).decode())

    # -- corpus / assignments ----------------------------------------------
    def set_corpus(self, m, doc_off, tokens):
        doc_off = np.ascontiguousarray(doc_off, dtype=np.int64)
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        if doc_off.ndim != 1 or len(doc_off) < 1 or len(tokens) != int(doc_off[-1]):
            raise ValueError("doc_off/tokens shape mismatch")
        self._ck(self.L.mvhdp_set_corpus(self.h, m, len(doc_off) - 1, _ptr(doc_off), _ptr(tokens)))
        self.D = len(doc_off) - 1
        self.N[m] = int(doc_off[-1])

    def set_assignments(self, m, z):
        z = np.ascontiguousarray(z, dtype=np.int32)
        if len(z) != self.N[m]:
            raise ValueError("z length mismatch")
        self._ck(self.L.mvhdp_set_assignments(self.h, m, _ptr(z)))

    def set_view_presence(self, m, present):
        """present: uint8 [D] (1 = the entity has the view even without tokens) or None (inferred from the spans)."""
        if present is None:
            self._ck(self.L.mvhdp_set_view_presence(self.h, m, None))
            return
        p = np.ascontiguousarray(present, dtype=np.uint8)
        if len(p) != self.D:
            raise ValueError("presence mask length mismatch")
        self._ck(self.L.mvhdp_set_view_presence(self.h, m, _ptr(p)))

    def get_assignments(self, m):
        z = np.empty(self.N[m], dtype=np.int32)
        self._ck(self.L.mvhdp_get_assignments(self.h, m, _ptr(z)))
        return z

    # -- model state --------------------------------------------------------
    def set_hyper(self, hy: Hyper):
        M, K = self.M, self.K
        hc = HyperC()
        self._alpha_keep = np.ascontiguousarray(hy.alpha, dtype=np.float64).reshape(M, K + 1)
        hc.alpha = self._alpha_keep.ctypes.data
        for m in range(M):
            hc.alpha_sum[m] = float(hy.alpha_sum[m]); hc.beta[m] = float(hy.beta[m])
            hc.beta_sum[m] = float(hy.beta_sum[m]); hc.gamma[m] = float(hy.gamma[m])
            for j in range(M):
                hc.p_a[m][j] = float(hy.p_a[m][j]); hc.p_b[m][j] = float(hy.p_b[m][j])
        self._inactive_keep = None
        if hy.inactive is not None:
            self._inactive_keep = np.ascontiguousarray(hy.inactive, dtype=np.uint8).reshape(K)
            hc.inactive = self._inactive_keep.ctypes.data
        self._ck(self.L.mvhdp_set_hyper(self.h, C.byref(hc)))

    def get_alpha(self):
        a = np.empty((self.M, self.K + 1), dtype=np.float64)
        ina = np.empty(self.K, dtype=np.uint8)
        self._ck(self.L.mvhdp_get_alpha(self.h, _ptr(a), _ptr(ina)))
        return a, ina

    def build_counts(self):
        self._ck(self.L.mvhdp_build_counts(self.h))

    def build_trees(self):
        self._ck(self.L.mvhdp_build_trees(self.h))

    def build_inference_trees(self):
        self._ck(self.L.mvhdp_build_inference_trees(self.h))

    def init_assignments_from_trees(self, seed):
        self._ck(self.L.mvhdp_init_assignments_from_trees(self.h, int(seed)))

    def get_counts(self, m):
        nwk = np.empty((self.V[m], self.K), dtype=np.int32)
        nk = np.empty(self.K, dtype=np.int32)
        self._ck(self.L.mvhdp_get_counts(self.h, m, _ptr(nwk), _ptr(nk)))
        return nwk, nk

    def set_counts(self, m, nwk, nk):
        nwk = np.ascontiguousarray(nwk, dtype=np.int32)
        nk = np.ascontiguousarray(nk, dtype=np.int32)
        assert nwk.shape == (self.V[m], self.K) and nk.shape == (self.K,)
        self._ck(self.L.mvhdp_set_counts(self.h, m, _ptr(nwk), _ptr(nk)))

    def get_tree(self, m, w):
        t = np.empty(2 * self.K, dtype=np.float64)
        self._ck(self.L.mvhdp_get_tree(self.h, m, w, _ptr(t)))
        return t

    def get_doc_topic_hist(self, m, hist_len, len_len=0):
        hist = np.empty((self.K, hist_len), dtype=np.int32)
        dl = np.empty(max(len_len, 1), dtype=np.int32) if len_len > 0 else None
        self._ck(self.L.mvhdp_get_doc_topic_hist(self.h, m, _ptr(hist), hist_len, _ptr(dl), len_len))
        return hist, (dl[:len_len] if dl is not None else None)

    # -- statistics either side of the sweep ------------------------
    def get_count_histogram(self, m, length):
        h = np.zeros(length, dtype=np.int32)
        self._ck(self.L.mvhdp_get_count_histogram(self.h, m, _ptr(h), length))
        return h

    def view_overlap_sums(self):
        s = np.zeros((self.M, self.M), dtype=np.float64)
        self._ck(self.L.mvhdp_view_overlap_sums(self.h, _ptr(s)))
        return s

    def model_log_likelihood(self):
        ll = np.zeros(self.M, dtype=np.float64)
        self._ck(self.L.mvhdp_model_log_likelihood(self.h, _ptr(ll)))
        return ll

    def gamma_doc_statistics(self, m, gamma_m, seed, round_idx):
        """PTM:2415-2433: (qs, qw) = (sum Bernoulli(j/(j+gamma)), sum log Beta(gamma+1, j)) over the entities with view m."""
        qs, qw = C.c_double(), C.c_double()
        self._ck(self.L.mvhdp_gamma_doc_statistics(self.h, int(m), float(gamma_m), int(seed), int(round_idx), C.byref(qs), C.byref(qw)))
        return qs.value, qw.value

    def doc_topic_proportions(self, view_weights, d0=0, d1=None):
        """PTM:2871-2899: [d1-d0][K] topic proportions, view_weights[m] = (m==0 ? 1 : discrWeight[m]) * pMean[0][m]."""
        d1 = self.D if d1 is None else int(d1)
        w = np.ascontiguousarray(view_weights, dtype=np.float64)
        out = np.zeros((max(d1 - int(d0), 0), self.K), dtype=np.float64)
        self._ck(self.L.mvhdp_doc_topic_proportions(self.h, _ptr(w), int(d0), d1, _ptr(out)))
        return out

    # -- after training: thresholded topic lists, entity distributions, all-pairs similarity (FLOW:246-260) --
    def doc_topics_top(self, view_weights, threshold, max_topics=-1, d0=0, d1=None):
        """PTM:2890-2926: (row_off [d1-d0+1], topics, weights) -- per entity the topics by weight descending (ties: larger topic id first),
        cut at the first weight < threshold and at max_topics (< 0 or > K: K).  Weights unrounded."""
        d0 = int(d0)
        d1 = self.D if d1 is None else int(d1)
        w = np.ascontiguousarray(view_weights, dtype=np.float64)
        if w.shape != (self.M,):
            raise ValueError("view_weights must be [M]")
        cnt = C.c_int64()
        off = np.zeros(max(d1 - d0, 0) + 1, dtype=np.int64)
        self._ck(self.L.mvhdp_doc_topics_top(self.h, _ptr(w), d0, d1, float(threshold), int(max_topics), 0, _ptr(off), None, None, C.byref(cnt)))
        n = cnt.value
        topics = np.zeros(n, dtype=np.int32)
        weights = np.zeros(n, dtype=np.float64)
        if n:
            self._ck(self.L.mvhdp_doc_topics_top(self.h, _ptr(w), d0, d1, float(threshold), int(max_topics), n, _ptr(off), _ptr(topics), _ptr(weights), C.byref(cnt)))
        return off, topics, weights

    def entity_topic_distributions(self, view_weights, threshold, groups, max_topics=-1, round_digits=5):
        """FLOW:807-1083 as include/mvhdp.h defines it: groups is a list of entity-id lists (or (member_off, members)); [n_groups][K]."""
        w = np.ascontiguousarray(view_weights, dtype=np.float64)
        if w.shape != (self.M,):
            raise ValueError("view_weights must be [M]")
        moff, mem = _member_csr(groups)
        ng = len(moff) - 1
        out = np.zeros((ng, self.K), dtype=np.float64)
        self._ck(self.L.mvhdp_entity_topic_distributions(self.h, _ptr(w), float(threshold), int(max_topics), int(round_digits), ng, _ptr(moff),
                                                         _ptr(mem) if len(mem) else None, _ptr(out) if ng else None))
        return out

    def similar_pairs(self, x, metric, threshold, min_weight=-np.inf, stripe_rows=0, candidate_capacity=0, count_only=False):
        """calcSimilarities FLOW:1320-1532 / CalcTopicSimilarities FLOW:1084-1196: all pairs i < j of the rows of x [n][dim] with
        sim > threshold, sorted by (i, j): (i, j, sim, stats).  metric: "cos_folded" (1 - |1 - cos|, the entity similarities), "cos" (the
        topic similarities) or "jsd", or the MVHDP_SIM_* value.  count_only: (count, stats)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("x must be [n][dim]")
        a = SimArgsC(int(SIM_METRICS.get(metric, metric)), x.shape[0], x.shape[1], x.ctypes.data, float(min_weight), float(threshold),
                     int(stripe_rows), int(candidate_capacity))
        cnt, st = C.c_int64(), SimStatsC()
        if count_only:
            self._ck(self.L.mvhdp_similar_pairs(self.h, C.byref(a), 0, None, None, None, C.byref(cnt), C.byref(st)))
            return cnt.value, _sim_stats(st)
        cap = 1 << 20                                          # a first guess; a call that finds more says how many and is repeated once
        while True:
            i, j, sim = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
            rc = self.L.mvhdp_similar_pairs(self.h, C.byref(a), cap, _ptr(i), _ptr(j), _ptr(sim), C.byref(cnt), C.byref(st))
            if rc == -1 and cnt.value > cap:
                cap = cnt.value
                continue
            self._ck(rc)
            n = cnt.value
            return i[:n].copy(), j[:n].copy(), sim[:n].copy(), _sim_stats(st)

    def topic_phrases_raw(self, max_per_topic=20, hash_bits=0):
        """mvhdp_topic_phrases as arrays: (topic_off [K+1], word_off [kept+1], words, counts [kept], distinct [K], occurrences [K], stats).
        Two calls, sizes then arrays (the walk runs twice, as for doc_topics_top)."""
        a = PhraseArgsC(int(max_per_topic), int(hash_bits))
        np_, nw, st = C.c_int64(), C.c_int64(), PhraseStatsC()
        topic_off = np.zeros(self.K + 1, dtype=np.int64)
        distinct = np.zeros(self.K, dtype=np.int64)
        occ = np.zeros(self.K, dtype=np.int64)
        self._ck(self.L.mvhdp_topic_phrases(self.h, C.byref(a), 0, 0, None, None, None, None, None, None, C.byref(np_), C.byref(nw), None))
        n, w = np_.value, nw.value
        word_off = np.zeros(n + 1, dtype=np.int64)
        words = np.zeros(w, dtype=np.int32)
        counts = np.zeros(n, dtype=np.int32)
        self._ck(self.L.mvhdp_topic_phrases(self.h, C.byref(a), n, w, _ptr(topic_off), _ptr(word_off), _ptr(words) if w else None, _ptr(counts),
                                            _ptr(distinct), _ptr(occ), C.byref(np_), C.byref(nw), C.byref(st)))
        return topic_off, word_off, words, counts, distinct, occ, PhraseStats(**{f: getattr(st, f) for f, _ in PhraseStatsC._fields_})

    def topic_phrases(self, max_per_topic=20, vocabulary=None, hash_bits=0):
        """findTopicPhrases PTM:1921-1976 on the device (what saveTopicsandExperiment stores, PTM:1555-1586, with max_per_topic = 20): a
        TopicPhrases.  vocabulary: the view-0 words, to get the reference's keys (the words joined by a blank) instead of word-id tuples."""
        topic_off, word_off, words, counts, distinct, occ, st = self.topic_phrases_raw(max_per_topic, hash_bits)
        phrases = []
        for k in range(self.K):
            row = []
            for p in range(int(topic_off[k]), int(topic_off[k + 1])):
                ids = tuple(int(x) for x in words[word_off[p]:word_off[p + 1]])
                row.append((ids if vocabulary is None else " ".join(str(vocabulary[i]) for i in ids), int(counts[p])))
            phrases.append(row)
        return TopicPhrases(phrases, distinct, occ, st)

    def heldout_left_to_right(self, doc_off, tokens, particles=10, resample=True, seed=0, m=0, doc_base=0, alpha=None, alpha_sum=None,
                              want_position_sums=False):
        """getMALLETProbEstimator().evaluateLeftToRight(testing, particles, resample, null) (PTM:3470-3478) on the device, as
        include/mvhdp.h defines it: a HeldoutResult.  The documents are passed here; a token >= V[m] is out of vocabulary.  alpha ([K])
        with alpha_sum replaces the handle's alpha[m] and gamma[m] * alphaSum[m]."""
        doc_off, tokens = _heldout_docs(doc_off, tokens)
        D, N = len(doc_off) - 1, len(tokens)
        a = HeldoutArgsC(int(m), int(particles), 1 if resample else 0, int(seed), int(doc_base), None, 0.0)
        keep = None
        if alpha is not None:
            keep = np.ascontiguousarray(alpha, dtype=np.float64)
            if keep.shape != (self.K,) or alpha_sum is None:
                raise ValueError("alpha: K values and alpha_sum, together")
            a.alpha, a.alpha_sum = keep.ctypes.data, float(alpha_sum)
        doc_ll = np.zeros(D, dtype=np.float64)
        pos = np.zeros(N, dtype=np.float64) if want_position_sums else None
        doc_tokens = np.zeros(D, dtype=np.int64)
        st = HeldoutStatsC()
        self._ck(self.L.mvhdp_heldout_left_to_right(self.h, C.byref(a), D, _ptr(doc_off), _ptr(tokens), _ptr(doc_ll), _ptr(pos), _ptr(doc_tokens), C.byref(st)))
        return HeldoutResult(st.log_likelihood, doc_ll, pos, doc_tokens, st.tokens, st.oov, st.visits, int(particles))

    def fold_in(self, doc_off, tokens, view_weights, iterations=10, samples=1, thin=1, seed=0, doc_base=0, coupling=None, want_z=False,
                want_counts=False):
        """The topic proportions of unseen documents against this handle's frozen counts (include/mvhdp.h mvhdp_fold_in): a FoldinResult
        whose theta rows go to nearest_entities(queries=...) and predict_items(theta=...) as they are.  doc_off and tokens: lists of
        length M, None for a view no document has; a token >= V[m] is out of vocabulary.  view_weights [M] as doc_topic_proportions
        takes them (None: no theta).  samples > 1 averages the states after the last `samples` iterations that lie `thin` apart.
        coupling: [M][M], how much of view i's topic mass view m's conditional sees (None: the mean of the handle's Beta(p_a, p_b))."""
        if len(doc_off) != self.M or len(tokens) != self.M:
            raise ValueError("doc_off and tokens: one entry per view (None for a view no document has)")
        offs, toks, D = [], [], None
        for o, t in zip(doc_off, tokens):
            if o is None:
                offs.append(None); toks.append(None)
                continue
            o, t = _heldout_docs(o, np.zeros(0, dtype=np.int32) if t is None else t)
            if D is not None and len(o) - 1 != D:
                raise ValueError("every view's doc_off must describe the same documents")
            D = len(o) - 1
            offs.append(o); toks.append(t)
        D = 0 if D is None else D
        a = FoldinArgsC(int(iterations), int(samples), int(thin), int(seed), int(doc_base), None, None)
        w = p = None
        if view_weights is not None:
            w = np.ascontiguousarray(view_weights, dtype=np.float64)
            if w.shape != (self.M,):
                raise ValueError("view_weights must be [M]")
            a.view_weights = w.ctypes.data
        if coupling is not None:
            p = np.ascontiguousarray(coupling, dtype=np.float64)
            if p.shape != (self.M, self.M):
                raise ValueError("coupling must be [M][M]")
            a.coupling = p.ctypes.data
        vpM = C.c_void_p * self.M
        theta = np.zeros((D, self.K), dtype=np.float64) if w is not None else None
        z = [None if o is None else np.full(len(t), -1, dtype=np.int32) for o, t in zip(offs, toks)] if want_z else None
        cs = np.zeros((D, self.M, self.K), dtype=np.int32) if want_counts else None
        c_off = vpM(*[None if o is None else o.ctypes.data for o in offs])
        c_tok = vpM(*[None if t is None else t.ctypes.data for t in toks])
        c_z = vpM(*[None if x is None else x.ctypes.data for x in z]) if want_z else None
        st = FoldinStatsC()
        self._ck(self.L.mvhdp_fold_in(self.h, C.byref(a), D, c_off, c_tok, _ptr(theta), c_z, _ptr(cs), C.byref(st)))
        return FoldinResult(theta, z, cs, st.tokens, st.oov, st.visits, st.kernel_ms)

    # -- cross-view prediction (include/mvhdp.h mvhdp_predict_items / mvhdp_score_items) --
    def _predict_args(self, m, view_weights, d0, d1, exclude_present, theta):
        d0 = int(d0)
        d1 = self.D if d1 is None else int(d1)
        a = PredictArgsC(int(m), 1 if exclude_present else 0, None, None)
        keep = []
        if view_weights is not None:
            w = np.ascontiguousarray(view_weights, dtype=np.float64)
            if w.shape != (self.M,):
                raise ValueError("view_weights must be [M]")
            keep.append(w)
            a.view_weights = w.ctypes.data
        if theta is not None:
            t = np.ascontiguousarray(theta, dtype=np.float64)
            if t.shape != (max(d1 - d0, 0), self.K):
                raise ValueError("theta must be [d1 - d0][K]")
            keep.append(t)
            a.theta = t.ctypes.data
        return a, keep, d0, d1

    def predict_items(self, m, view_weights, n, d0=0, d1=None, exclude_present=True, theta=None):
        """The first n types of view m per entity of [d0, d1) by score(d, w) = sum_k theta_d[k] phi_m[w][k], score descending, equal
        scores by type id: (items [d1-d0][n] (-1 unfilled), scores [d1-d0][n], counts [d1-d0]).  theta_d is
        doc_topic_proportions(view_weights) -- pass view_weights[m] = 0 to predict the view from the others -- or the rows of theta.
        exclude_present: the types the entity already holds in view m are not listed."""
        a, keep, d0, d1 = self._predict_args(m, view_weights, d0, d1, exclude_present, theta)
        n = int(n)
        rows = max(d1 - d0, 0)
        items = np.full((rows, max(n, 0)), -1, dtype=np.int32)
        scores = np.zeros((rows, max(n, 0)), dtype=np.float64)
        counts = np.zeros(rows, dtype=np.int32)
        self._ck(self.L.mvhdp_predict_items(self.h, C.byref(a), d0, d1, n, _ptr(items), _ptr(scores), _ptr(counts)))
        return items, scores, counts

    def score_items(self, m, view_weights, entities, items, d0=0, d1=None, exclude_present=True, theta=None):
        """Score and rank given (entity, item) pairs of view m -- the held-back items of a held-out evaluation: an ItemScores.  Entities
        are ids of this handle inside [d0, d1), in any order, repeats allowed; rank counts the types that are not excluded for the
        entity and come before the item (the item itself is ranked even if the entity holds it)."""
        a, keep, d0, d1 = self._predict_args(m, view_weights, d0, d1, exclude_present, theta)
        ent = np.ascontiguousarray(entities, dtype=np.int64)
        it = np.ascontiguousarray(items, dtype=np.int32)
        if ent.ndim != 1 or ent.shape != it.shape:
            raise ValueError("entities and items: two arrays of one length")
        score = np.zeros(len(ent), dtype=np.float64)
        rank = np.zeros(len(ent), dtype=np.int32)
        self._ck(self.L.mvhdp_score_items(self.h, C.byref(a), d0, d1, len(ent), _ptr(ent), _ptr(it), _ptr(score), _ptr(rank)))
        return ItemScores(score, rank)

    # -- entities for an item (include/mvhdp.h mvhdp_predict_entities / mvhdp_rank_entities) --
    def _entities_args(self, m, view_weights, items, weights, psi, c0, c1, exclude_present, block_entities, block_queries):
        w = np.ascontiguousarray(view_weights, dtype=np.float64)
        if w.shape != (self.M,):
            raise ValueError("view_weights must be [M]")
        c1 = self.D if c1 is None else int(c1)
        a = EntitiesArgsC(int(m), 1 if exclude_present else 0, w.ctypes.data, int(c0), c1, 0, None, None, None, None, int(block_entities), int(block_queries))
        keep = [w]
        if psi is not None:
            if items is not None or weights is not None:
                raise ValueError("either items (with weights) or psi")
            x = np.ascontiguousarray(psi, dtype=np.float64)
            if x.ndim != 2 or x.shape[1] != self.K:
                raise ValueError("psi must be [nq][K]")
            keep.append(x)
            a.psi, a.nq = x.ctypes.data, x.shape[0]
            return a, keep
        if items is None:
            raise ValueError("neither items nor psi")
        one = isinstance(items, np.ndarray) and items.ndim == 1              # one item per query
        lists = [[int(i)] for i in items] if one else [list(q) for q in items]
        off = np.concatenate([[0], np.cumsum([len(q) for q in lists])]).astype(np.int64)
        flat = np.ascontiguousarray([i for q in lists for i in q], dtype=np.int32)
        keep += [off, flat]
        a.nq, a.q_off, a.q_items = len(lists), off.ctypes.data, flat.ctypes.data if len(flat) else None
        if weights is not None:
            wl = [[float(x)] for x in weights] if one else [list(q) for q in weights]
            if [len(q) for q in wl] != [len(q) for q in lists]:
                raise ValueError("weights: one per item")
            fw = np.ascontiguousarray([x for q in wl for x in q], dtype=np.float64)
            keep.append(fw)
            a.q_weights = fw.ctypes.data if len(fw) else None
        return a, keep

    def predict_entities(self, m, view_weights, n, items=None, weights=None, psi=None, c0=0, c1=None, exclude_present=True, block_entities=0, block_queries=0):
        """Per query the first n (<= 1024) entities of [c0, c1) by score(d, j) = sum_k theta_d[k] psi_j[k], score descending, equal scores
        by entity id: an EntityRanking.  Queries: `items`, a list of lists of types of view m (or a 1-D array: one item per query) with
        optional `weights` of the same shape -- psi_j is the weighted sum of their phi rows -- or `psi`, rows [nq][K] of the caller's.
        theta_d is doc_topic_proportions(view_weights), formed on the device; pass view_weights[m] = 0 to predict the view from the
        others.  exclude_present (item form): an entity whose view-m span holds an item of the query is not listed.  For a one-item
        query every score has the bits of score_items for the same (entity, item).  block_entities, block_queries: work sizes (0: auto)."""
        a, keep = self._entities_args(m, view_weights, items, weights, psi, c0, c1, exclude_present, block_entities, block_queries)
        n = int(n)
        nq = int(a.nq)
        ids = np.full((nq, max(n, 0)), -1, dtype=np.int64)
        scores = np.zeros((nq, max(n, 0)), dtype=np.float64)
        counts = np.zeros(nq, dtype=np.int32)
        st = EntitiesStatsC()
        self._ck(self.L.mvhdp_predict_entities(self.h, C.byref(a), n, _ptr(ids), _ptr(scores), _ptr(counts), C.byref(st)))
        return EntityRanking(ids, scores, counts, EntitiesStats(st.cells, st.excluded, st.blocks, st.kernel_ms))

    def rank_entities(self, m, view_weights, queries, entities, items=None, weights=None, psi=None, c0=0, c1=None, exclude_present=True,
                      block_entities=0, block_queries=0):
        """Score and rank given (query index, entity) pairs -- the held-back links of an evaluation from the item's side: an EntityRanks.
        rank counts the candidates of [c0, c1) that are not excluded for the query and come before the entity (the entity itself is
        ranked even if it is excluded).  Pairs may repeat and come in any order."""
        a, keep = self._entities_args(m, view_weights, items, weights, psi, c0, c1, exclude_present, block_entities, block_queries)
        qi = np.ascontiguousarray(queries, dtype=np.int64)
        ent = np.ascontiguousarray(entities, dtype=np.int64)
        if qi.ndim != 1 or qi.shape != ent.shape:
            raise ValueError("queries and entities: two arrays of one length")
        score = np.zeros(len(qi), dtype=np.float64)
        rank = np.zeros(len(qi), dtype=np.int64)
        self._ck(self.L.mvhdp_rank_entities(self.h, C.byref(a), len(qi), _ptr(qi), _ptr(ent), _ptr(score), _ptr(rank)))
        return EntityRanks(score, rank)

    # -- retrieval (include/mvhdp.h mvhdp_nearest_entities / mvhdp_topic_top_entities) --
    def nearest_entities(self, view_weights, n, queries=None, q0=0, q1=None, c0=0, c1=None, exclude_self=True, min_weight=-np.inf,
                         block_queries=0, stripe_candidates=0, candidate_capacity=0):
        """Per query row the n entities of [c0, c1) with the largest cosine similarity of their topic proportions
        (doc_topic_proportions(view_weights), formed on the device), sim descending, equal sims by entity id: a NearestResult.  Queries:
        the rows of `queries` [nq][K] -- the proportions of folded-in documents, say -- or, without them, the entities [q0, q1) of this
        handle, each left out of its own list unless exclude_self is False.  An entry <= min_weight counts as 0.  Every sim has the bits
        of similar_pairs(.., "cos", ..) for the same pair.  block_queries, stripe_candidates, candidate_capacity: work sizes (0: auto)."""
        w = np.ascontiguousarray(view_weights, dtype=np.float64)
        if w.shape != (self.M,):
            raise ValueError("view_weights must be [M]")
        n = int(n)
        c1 = self.D if c1 is None else int(c1)
        q1 = self.D if q1 is None else int(q1)
        a = NearestArgsC(w.ctypes.data, int(c0), c1, None, 0, int(q0), q1, 1 if exclude_self else 0, n, float(min_weight),
                         int(block_queries), int(stripe_candidates), int(candidate_capacity))
        x = None
        if queries is not None:
            x = np.ascontiguousarray(queries, dtype=np.float64)
            if x.ndim != 2 or x.shape[1] != self.K:
                raise ValueError("queries must be [nq][K]")
            a.queries, a.nq = x.ctypes.data, x.shape[0]
        nq = x.shape[0] if x is not None else max(q1 - int(q0), 0)
        ids = np.full((nq, max(n, 0)), -1, dtype=np.int64)
        sims = np.zeros((nq, max(n, 0)), dtype=np.float64)
        counts = np.zeros(nq, dtype=np.int32)
        st = NearestStatsC()
        self._ck(self.L.mvhdp_nearest_entities(self.h, C.byref(a), _ptr(ids), _ptr(sims), _ptr(counts), C.byref(st)))
        return NearestResult(ids, sims, counts, _nearest_stats(st))

    def topic_top_entities(self, view_weights, n, threshold=-np.inf, d0=0, d1=None, chunk_entities=0, slice_entities=0):
        """Per topic the n (<= 1024) entities of [d0, d1) with the largest proportion > threshold, weight descending, equal weights by
        entity id: (ids [K][n] (-1 unfilled), weights [K][n], counts [K]).  chunk_entities, slice_entities: work sizes (0: auto)."""
        w = np.ascontiguousarray(view_weights, dtype=np.float64)
        if w.shape != (self.M,):
            raise ValueError("view_weights must be [M]")
        n = int(n)
        d1 = self.D if d1 is None else int(d1)
        ids = np.full((self.K, max(n, 0)), -1, dtype=np.int64)
        weights = np.zeros((self.K, max(n, 0)), dtype=np.float64)
        counts = np.zeros(self.K, dtype=np.int32)
        self._ck(self.L.mvhdp_topic_top_entities(self.h, _ptr(w), int(d0), d1, n, float(threshold), int(chunk_entities), int(slice_entities),
                                                 _ptr(ids), _ptr(weights), _ptr(counts)))
        return ids, weights, counts

    # -- the topic map (include/mvhdp.h mvhdp_topic_gram) --
    def topic_gram(self, source, m=0, view_weights=None, r0=0, r1=None, transform="identity", threshold=None, blocks_per_pass=0):
        """K x K sums over the rows of `source`: "entities" (theta of the entities [r0, r1), doc_topic_proportions(view_weights), formed
        on the device), "words" (phi of view m over the types [r0, r1)) or an ndarray [n][K] of the caller's (finite, >= 0; r0 and r1
        cut it).  transform "identity" or "sqrt".  A TopicGram: gram and sums in the contract's fixed order (blocks of 1024 rows, one fma
        chain per block and cell, the blocks added in ascending order), and with a `threshold` the exact counts n_above and co_above of
        the rows with X > threshold (strictly; taken before the transform).  blocks_per_pass: a work size (0: auto); it changes no result."""
        srcs = {"entities": 0, "words": 1}
        tr = {"identity": 0, "sqrt": 1}
        if transform not in tr:
            raise ValueError('transform must be "identity" or "sqrt"')
        keep = []
        a = TopicGramArgsC(0, int(m), tr[transform], int(blocks_per_pass), None, None, int(r0), 0, 0.0 if threshold is None else float(threshold))
        if isinstance(source, str):
            if source not in srcs:
                raise ValueError('source must be "entities", "words" or an array [n][K]')
            a.source = srcs[source]
            a.r1 = (self.D if source == "entities" else int(self.V[int(m)])) if r1 is None else int(r1)
            if source == "entities":
                w = np.ascontiguousarray(view_weights, dtype=np.float64)
                if w.shape != (self.M,):
                    raise ValueError("view_weights must be [M]")
                keep.append(w)
                a.view_weights = w.ctypes.data
        else:
            x = np.ascontiguousarray(source, dtype=np.float64)
            if x.ndim != 2 or x.shape[1] != self.K:
                raise ValueError("source rows must be [n][K]")
            r1 = x.shape[0] if r1 is None else int(r1)
            if not 0 <= int(r0) <= r1 <= x.shape[0]:
                raise ValueError("bad row range")
            x = np.ascontiguousarray(x[int(r0):r1]) if r1 > int(r0) else np.zeros((1, self.K))
            keep.append(x)
            a.source, a.x, a.r1 = 2, x.ctypes.data, r1
        gram = np.zeros((self.K, self.K), dtype=np.float64)
        sums = np.zeros(self.K, dtype=np.float64)
        n_above = co_above = None
        if threshold is not None:
            n_above = np.zeros(self.K, dtype=np.int64)
            co_above = np.zeros((self.K, self.K), dtype=np.int64)
        st = TopicGramStatsC()
        self._ck(self.L.mvhdp_topic_gram(self.h, C.byref(a), _ptr(gram), _ptr(sums), None if n_above is None else _ptr(n_above),
                                         None if co_above is None else _ptr(co_above), C.byref(st)))
        return TopicGram(gram, sums, n_above, co_above, int(st.rows), transform, TopicGramStats(st.rows, st.blocks, st.passes, st.kernel_ms))

    # -- topic words per cohort (include/mvhdp.h mvhdp_cohort_top_words) --
    def cohort_top_words(self, m, cohorts, n=20, order="count", min_count=1, trends_only=False, scratch_bytes=0):
        """A topic's words inside sets of entities: cohorts is a list of entity-id lists (or (member_off, members)), as the groups of
        entity_topic_distributions; an entity may be listed in several cohorts and more than once, every listing counts.  A CohortWords:
        per cohort and topic the top n types of view m by their count inside the cohort (order "count", the order of top_words) or by
        the exact share of the word's topic tokens that lies in the cohort (order "share"; needs current counts), among the types with
        at least min_count tokens there; tokens and docs are the trend in token and in listing units.  trends_only: tokens and docs
        alone, without a count table.  scratch_bytes bounds the device scratch of the count tables (0: auto); it changes no result."""
        orders = {"count": COHORT_BY_COUNT, "share": COHORT_BY_SHARE}
        if order not in orders:
            raise ValueError('order must be "count" or "share"')
        moff, mem = _member_csr(cohorts)
        G, n = len(moff) - 1, int(n)
        a = CohortArgsC(int(m), n, orders[order], int(min_count), int(scratch_bytes))
        types = counts = nonzero = None
        if not trends_only:
            types = np.full((G, self.K, max(n, 1)), -1, dtype=np.int32)
            counts = np.zeros((G, self.K, max(n, 1)), dtype=np.int32)
            nonzero = np.zeros((G, self.K), dtype=np.int32)
        tokens = np.zeros((G, self.K), dtype=np.int64)
        docs = np.zeros((G, self.K), dtype=np.int64)
        st = CohortStatsC()
        self._ck(self.L.mvhdp_cohort_top_words(self.h, C.byref(a), G, _ptr(moff), _ptr(mem) if len(mem) else None, _ptr(types), _ptr(counts),
                                               _ptr(nonzero), _ptr(tokens), _ptr(docs), C.byref(st)))
        return CohortWords(types, counts, nonzero, tokens, docs, CohortStats(**{f: getattr(st, f) for f, _ in CohortStatsC._fields_}))

    # -- word-set co-occurrence (include/mvhdp.h mvhdp_word_cooccurrence) --
    def word_cooccurrence(self, sets, m=0, window=0, d0=0, d1=None, corpus=None) -> WordCooccurrence:
        """In how many windows the words of each set occur, alone and in pairs: sets is an int array [S][n] or a list of lists (padded
        with -1 to the longest), e.g. top_words(m, n)[0].  window 0: one window per entity (document co-occurrence); W >= 1: the Boolean
        sliding window of W positions.  corpus: None for view m as the handle holds it, or (doc_off, tokens) of a held-out or reference
        corpus of that view; the assignments are never read.  Only the entities [d0, d1) are counted (d1 None: to the end).  The measures
        (uci, npmi, umass) are methods of the WordCooccurrence returned."""
        st_sets = _word_sets(sets)
        S, n = st_sets.shape
        doc_off = tokens = None
        num_docs = 0
        if corpus is not None:
            doc_off, tokens = _heldout_docs(*corpus)
            num_docs = len(doc_off) - 1
        a = CoocArgsC(int(m), int(n), int(window), int(d0), -1 if d1 is None else int(d1))
        co = np.zeros((S, n, n), dtype=np.int64)
        windows = np.zeros(1, dtype=np.int64)
        st = CoocStatsC()
        self._ck(self.L.mvhdp_word_cooccurrence(self.h, C.byref(a), S, _ptr(st_sets) if st_sets.size else None, num_docs, _ptr(doc_off),
                                                _ptr(tokens) if tokens is not None and len(tokens) else None, _ptr(co), _ptr(windows), C.byref(st)))
        return WordCooccurrence(co, int(windows[0]), st_sets, CoocStats(**{f: getattr(st, f) for f, _ in CoocStatsC._fields_}))

    def topic_coherence(self, n=20, m=0, window=0, measure="npmi", corpus=None):
        """[K] float64: top_words(m, n) into word_cooccurrence into WordCooccurrence.coherence(measure), one value per topic (NaN for a
        topic without two words that occur).  Needs current counts, as top_words does."""
        return self.word_cooccurrence(self.top_words(m, n)[0], m, window, corpus=corpus).coherence(measure)

    # -- topic diagnostics (FastQMVWVTopicModelDiagnostics; include/mvhdp.h mvhdp_top_words / _discr_weights / _diagnostics) --
    # -- topic surgery (include/mvhdp.h mvhdp_remap_topics; mvtopicmodel_amd/surgery.py builds the maps) --
    def remap_topics(self, topic_map, retire=False) -> RemapStats:
        """Merge, drop and reorder topics in place: topic_map [K], map[k] = the topic that takes topic k's tokens, -1 = they become
        unassigned; one hop, never chased.  The assignments, the counts, alpha and the inactive set move together and every kind of sweep
        goes on afterwards.  retire: the topics nothing maps onto join the inactive set, so that a later birth can take their index."""
        rc, st = _remap_call(self.L.mvhdp_remap_topics, self.h, self.K, self.M, topic_map, retire)
        self._ck(rc)
        return st

    def split_topic(self, source, target=None, iterations=20, seed=0, coupling=None, type_hint=None, keep_alpha=False) -> SplitStats:
        """Cut topic `source` in two in place (include/mvhdp.h mvhdp_split_topic): a Gibbs sampler restricted to the tokens of the source
        and to the two outcomes "stays" and "goes to target".  target: a free topic index (no token, alpha 0.0 in every view), None = the
        lowest free index of the inactive set (surgery.free_topics lists them).  type_hint: None, or per view None or an int8 row [V_m]
        (-1 none, 0 stays in source, 1 starts in target; surgery.hint_from_words builds one).  coupling: [M][M] as for fold_in.  alpha of
        the source is halved between the two unless keep_alpha.  Every kind of sweep goes on afterwards."""
        iterations = int(iterations)
        P = None if coupling is None else np.ascontiguousarray(coupling, dtype=np.float64)
        if P is not None and P.shape != (self.M, self.M):
            raise ValueError(f"split_topic: coupling must be [{self.M}][{self.M}], got {P.shape}")
        rows, hp = None, None
        if type_hint is not None:
            if len(type_hint) != self.M:
                raise ValueError(f"split_topic: type_hint must hold one entry per view ({self.M})")
            rows = [None if r is None else np.ascontiguousarray(r, dtype=np.int8) for r in type_hint]
            for m, r in enumerate(rows):
                if r is not None and r.shape != (self.V[m],):
                    raise ValueError(f"split_topic: type_hint[{m}] must hold one entry per type ({self.V[m]}), got shape {r.shape}")
            hp = (C.c_void_p * self.M)(*[None if r is None else r.ctypes.data for r in rows])
        a = SplitArgsC(int(source), -1 if target is None else int(target), iterations, SPLIT_KEEP_ALPHA if keep_alpha else 0, int(seed),
                       None if P is None else P.ctypes.data, None if hp is None else C.cast(hp, C.c_void_p))
        flips = np.zeros(max(iterations, 1), dtype=np.int64)
        st = SplitStatsC()
        self._ck(self.L.mvhdp_split_topic(self.h, C.byref(a), _ptr(flips), C.byref(st)))
        return SplitStats(np.array(st.split[:self.M], dtype=np.int64), np.array(st.moved[:self.M], dtype=np.int64), st.flips_last, st.target,
                          bool(st.activated), st.kernel_ms, flips[:max(iterations, 0)].copy())

    def top_words(self, m, n):
        """getSortedWords(m) PTM:1792-1811 cut at n: (types [K][n] (-1 unfilled), counts [K][n], nonzero [K])."""
        n = int(n)
        nn = max(n, 1)
        t = np.zeros((self.K, nn), np.int32)
        c = np.zeros((self.K, nn), np.int32)
        z = np.zeros(self.K, np.int32)
        self._ck(self.L.mvhdp_top_words(self.h, int(m), n, _ptr(t), _ptr(c), _ptr(z)))
        return t, c, z

    def discr_weights(self, m=None):
        """calcDiscrWeightAcrossTopicsPerModality PTM:2181-2230: discrWeightPerModality [M]; with a view m also typeDiscrWeight[m] [V_m]."""
        pv = np.zeros(self.M, dtype=np.float64)
        tw = None if m is None else np.zeros(self.V[int(m)], dtype=np.float64)
        self._ck(self.L.mvhdp_discr_weights(self.h, _ptr(pv), 0 if m is None else int(m), _ptr(tw)))
        return pv if m is None else (pv, tw)

    def diagnostics(self, num_top_words=20, vocabulary=None, word_length=None):
        """FastQMVWVTopicModelDiagnostics(model, num_top_words) DIAG:53-117 on the device.  vocabulary: the view-0 words (their Java
        String.length() feeds the word-length row), or word_length [V_0] directly; neither: that row is NaN."""
        rc, d = _run_diagnostics(self.L, self.L.mvhdp_diagnostics, self.h, self.K, self.V[0], self.M, num_top_words, vocabulary, word_length)
        self._ck(rc)
        return d

    # -- word and topic embeddings (TopicWordEmbeddings; include/mvhdp.h mvhdp_emb_*) ---------------------------------
    def emb_init(self, cfg: EmbConfig, weights=None, seed=0):
        """new TopicWordEmbeddings (TWE:126-163): rows V_0 words (+ K topics with cfg.with_topics), C columns."""
        c = cfg.to_c()
        rows = self.V[0] + (self.K if cfg.with_topics else 0)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if w is not None and w.shape != (rows, cfg.num_columns):
            raise ValueError(f"weights must be [{rows}][{cfg.num_columns}]")
        self._emb_shape = None
        self._ck(self.L.mvhdp_emb_init(self.h, C.byref(c), _ptr(w), int(seed)))
        self._emb_shape = (rows, int(cfg.num_columns), int(self.K if cfg.with_topics else 0))

    def _emb_dims(self):
        """(rows, columns, topic rows) of the embeddings; MvhdpError(STATE) as the library gives it before emb_init."""
        if getattr(self, "_emb_shape", None) is None:
            raise MvhdpError(-2, "embeddings: mvhdp_emb_init has not been called")
        return self._emb_shape

    def emb_count_words(self):
        """countWords(data, f) TWE:341-401 over view 0 (cumulative)."""
        self._ck(self.L.mvhdp_emb_count_words(self.h))

    def emb_train(self, epochs, seed, round_idx=0, serial=False) -> EmbStats:
        """train(data, threads, num_samples, epochs) TWE:423-483; serial: one wave in entity order (deterministic)."""
        st = EmbStatsC()
        self._ck(self.L.mvhdp_emb_train(self.h, int(epochs), int(seed), int(round_idx), EMB_SERIAL if serial else 0, C.byref(st)))
        return EmbStats(**{f: getattr(st, f) for f, _ in EmbStatsC._fields_})

    def emb_get_vectors(self):
        """(weights, negative_weights), each [R][C]: word rows, then topic rows (getWordVectors / getTopicVectors)."""
        R, ncol, _ = self._emb_dims()
        w = np.empty((R, ncol), dtype=np.float64)
        n = np.empty((R, ncol), dtype=np.float64)
        self._ck(self.L.mvhdp_emb_get_vectors(self.h, _ptr(w), _ptr(n)))
        return w, n

    def emb_set_vectors(self, weights=None, negative_weights=None):
        R, ncol, _ = self._emb_dims()
        a = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (weights, negative_weights)]
        for x in a:
            if x is not None and x.shape != (R, ncol):
                raise ValueError(f"vectors must be [{R}][{ncol}]")
        self._ck(self.L.mvhdp_emb_set_vectors(self.h, _ptr(a[0]), _ptr(a[1])))

    def emb_word_stats(self):
        """(cumulative wordCounts [V_0] int64, retentionProbability [V_0], totalWords)."""
        self._emb_dims()
        c = np.empty(self.V[0], dtype=np.int64)
        r = np.empty(self.V[0], dtype=np.float64)
        t = C.c_int64()
        self._ck(self.L.mvhdp_emb_word_stats(self.h, _ptr(c), _ptr(r), C.byref(t)))
        return c, r, t.value

    def emb_sampling_table(self, first, n):
        out = np.empty(int(n), dtype=np.int32)
        self._ck(self.L.mvhdp_emb_sampling_table(self.h, int(first), int(n), _ptr(out)))
        return out

    def emb_softmax(self, reset_sums=False, want_exp=True):
        """CalcSoftmaxTopicWordProbabilities PTM:337-367: (expDotProductValues [K][V_0] or None, sumExpValues [K], accumulated)."""
        _, _, K = self._emb_dims()
        e = np.empty((K, self.V[0]), dtype=np.float64) if want_exp else None
        s = np.empty(K, dtype=np.float64)
        self._ck(self.L.mvhdp_emb_softmax(self.h, 1 if reset_sums else 0, _ptr(e), _ptr(s)))
        return e, s

    def emb_nearest(self, query, n=10):
        """findClosest TWE:485-540: (words [n], word cosines [n], topics [n], topic cosines [n]) in IDSorter order."""
        q = np.ascontiguousarray(query, dtype=np.float64)
        w, ws = np.empty(int(n), np.int32), np.empty(int(n), np.float64)
        t, ts = np.full(int(n), -1, np.int32), np.full(int(n), np.nan)
        self._ck(self.L.mvhdp_emb_nearest(self.h, _ptr(q), int(n), _ptr(w), _ptr(ws), _ptr(t), _ptr(ts)))
        return w, ws, t, ts

    def emb_release(self):
        self._ck(self.L.mvhdp_emb_release(self.h))
        self._emb_shape = None

    # -- useVectorsLambda: the embeddings' p(w|t) mixed into the view-0 sampler (WRK:504-507, PTM:2673-2678) ------
    def set_vectors_mix(self, lam, exp_dot=None, sum_exp=None):
        """lam = 0: off.  0 < lam <= 1: on, with the host's expDotProductValues [K][V_0] / sumExpValues [K], or (both None) the
        handle's own softmax table as the last emb_softmax left it.  Invalidates the F+trees."""
        if (exp_dot is None) != (sum_exp is None):
            raise ValueError("exp_dot and sum_exp go together")
        e = s = None
        if exp_dot is not None:
            e = np.ascontiguousarray(exp_dot, dtype=np.float64)
            s = np.ascontiguousarray(sum_exp, dtype=np.float64)
            if e.shape != (self.K, self.V[0]) or s.shape != (self.K,):
                raise ValueError(f"exp_dot must be [{self.K}][{self.V[0]}] and sum_exp [{self.K}]")
        self._ck(self.L.mvhdp_set_vectors_mix(self.h, float(lam), _ptr(e), _ptr(s)))

    def get_vectors_mix(self, want_table=True):
        """(lambda, the device's table lambda * (e / S) as [V_0][K], or None when the mix is off or want_table is False)."""
        lam = C.c_double()
        self._ck(self.L.mvhdp_get_vectors_mix(self.h, C.byref(lam), None))
        if lam.value == 0.0 or not want_table:
            return lam.value, None
        t = np.empty((self.V[0], self.K), dtype=np.float64)
        self._ck(self.L.mvhdp_get_vectors_mix(self.h, None, _ptr(t)))
        return lam.value, t

    # -- the hot path ---------------------------------------------------------
    def sweep(self, sweep_idx, seed, flags=0, p=None, want_dbg=False, trace=None) -> SweepStats:
        st = SweepStatsC()
        if p is not None:
            p = np.ascontiguousarray(p, dtype=np.float64)
            if p.shape != (self.D, self.M, self.M):
                raise ValueError("p override must be [D][M][M]")
        dbgc = None
        dbg_arrays = None
        tout = None
        keep = []
        if want_dbg or trace:
            dbgc = DebugC()
            if want_dbg:
                dbg_arrays = [np.zeros((max(self.N[m], 1), 4), dtype=np.float64) for m in range(self.M)]
                for m in range(self.M):
                    dbgc.tok_dbg[m] = dbg_arrays[m].ctypes.data
            if trace:
                td = np.ascontiguousarray([t[0] for t in trace], dtype=np.int64)
                tv = np.ascontiguousarray([t[1] for t in trace], dtype=np.int32)
                tp = np.ascontiguousarray([t[2] for t in trace], dtype=np.int32)
                tout = np.zeros((len(trace), self.K + 1), dtype=np.float64)
                keep += [td, tv, tp]
                dbgc.n_trace = len(trace)
                dbgc.trace_doc = td.ctypes.data; dbgc.trace_view = tv.ctypes.data
                dbgc.trace_pos = tp.ctypes.data; dbgc.trace_out = tout.ctypes.data
        rc = self.L.mvhdp_sweep(self.h, int(sweep_idx), int(seed), int(flags), _ptr(p),
                                C.byref(dbgc) if dbgc is not None else None, C.byref(st))
        self._ck(rc)
        out = SweepStats(**{f: getattr(st, f) for f, _ in SweepStatsC._fields_})
        if dbg_arrays is not None:
            out.dbg = [a[: self.N[m]] for m, a in enumerate(dbg_arrays)]
        out.trace = tout
        return out

    def sweep_many(self, first_idx, n, seed, flags=0):
        """n sweeps enqueued back to back, one synchronisation (mvhdp_sweep_many): the list of their statistics."""
        arr = (SweepStatsC * max(int(n), 1))()
        self._ck(self.L.mvhdp_sweep_many(self.h, int(first_idx), int(n), int(seed), int(flags), C.cast(arr, C.c_void_p)))
        return [SweepStats(**{f: getattr(arr[i], f) for f, _ in SweepStatsC._fields_}) for i in range(int(n))]

    def sweep_census(self, enable=None, reset=False):
        """The launch census (mvhdp_sweep_census): one CensusRow per compiled sweep kernel -- its key (rmax, debug, walk, narrow, roomy,
        liverows, mix; rmax 0: the generic kernel), the launches it got and the tokens they sampled since the last reset.
        enable True / False switches the census of this handle on / off, None leaves it; the rows are read after the reset."""
        n = C.c_int32(0)
        self._ck(self.L.mvhdp_sweep_census(self.h, -1, 0, None, 0, C.byref(n)))
        arr = (CensusRowC * n.value)()
        self._ck(self.L.mvhdp_sweep_census(self.h, -1 if enable is None else int(bool(enable)), int(bool(reset)), arr, n.value, None))
        return [CensusRow((r.rmax, r.debug, r.walk, r.narrow, r.roomy, r.liverows, r.mix), r.launches, r.tokens) for r in arr]

    # -- tuning (never changes a result) --------------------------------------------
    def get_tuning(self):
        t = TuningC()
        self._ck(self.L.mvhdp_get_tuning(self.h, C.byref(t)))
        return t

    def set_tuning(self, t=None, **kw):
        """set_tuning(force_primary=2, walk_theta=[0.5, 0], narrow=0, ...): fields not named keep their value."""
        if t is None:
            t = self.get_tuning()
        for k, v in kw.items():
            if k in ("walk_theta", "tree_branch_share", "learnt_walk_step"):
                arr = getattr(t, k)
                for i, x in enumerate(v):
                    arr[i] = x
                if k == "walk_theta":
                    for i in range(len(v), MAX_M):
                        arr[i] = 0.0
            else:
                setattr(t, k, v)
        self._ck(self.L.mvhdp_set_tuning(self.h, C.byref(t)))

    def dp_table_statistics(self, m, hist, conc, seed, round_idx):
        """optimizeDP's view-table simulation on the device (mvhdp_dp_table_statistics): (mk [K], active [K])."""
        hist = np.ascontiguousarray(hist, dtype=np.int32)
        conc = np.ascontiguousarray(conc, dtype=np.float64)
        mk = np.zeros(self.K, dtype=np.float64); act = np.zeros(self.K, dtype=np.uint8)
        self._ck(self.L.mvhdp_dp_table_statistics(self.h, int(m), _ptr(hist), int(hist.shape[1]), _ptr(conc), int(seed), int(round_idx), _ptr(mk), _ptr(act)))
        return mk, act

    def antoniak_draws(self, items, conc, seed, round_idx):
        """n independent draws of the number of tables a CRP(conc[j]) makes of items[j] items (mvhdp_antoniak_draws)."""
        items = np.ascontiguousarray(items, dtype=np.int32); conc = np.ascontiguousarray(conc, dtype=np.float64)
        out = np.zeros(len(items), dtype=np.int32)
        self._ck(self.L.mvhdp_antoniak_draws(self.h, len(items), _ptr(items), _ptr(conc), int(seed), int(round_idx), _ptr(out)))
        return out

    def apply_delta(self, activated_topic=-1, activated_modality=-1):
        self._ck(self.L.mvhdp_apply_delta(self.h, int(activated_topic), int(activated_modality)))

    def apply_delta_begin(self):
        self._ck(self.L.mvhdp_apply_delta_begin(self.h))

    def apply_delta_rows(self, row_begin, row_end):
        self._ck(self.L.mvhdp_apply_delta_rows(self.h, int(row_begin), int(row_end)))

    def apply_delta_end(self, activated_topic=-1, activated_modality=-1):
        self._ck(self.L.mvhdp_apply_delta_end(self.h, int(activated_topic), int(activated_modality)))

    def get_birth_keys(self):
        """MVHDP_BUF_BIRTH_KEYS after a NO_APPLY sweep: int64 [K], the first delta that reached each topic that was inactive (SWEEP_SHARD_BIRTHS:
        every topic the shard gave birth to), ACT_KEY_NONE elsewhere."""
        keys = np.empty(self.K, dtype=np.int64)
        self._ck(self.L.mvhdp_get_birth_keys(self.h, _ptr(keys)))
        return keys

    def activate_births(self, keys=None):
        """Activates every topic whose key is not ACT_KEY_NONE (after apply_delta(-1, -1)); keys: int64 [K] (the MIN over all shards' tables),
        or None for MVHDP_BUF_BIRTH_KEYS as it stands on the device."""
        if keys is not None:
            keys = np.ascontiguousarray(keys, dtype=np.int64)
            if keys.shape != (self.K,):
                raise ValueError(f"activate_births: keys must have shape ({self.K},)")
        self._ck(self.L.mvhdp_activate_births(self.h, _ptr(keys)))

    def trees_current(self):
        rc = self.L.mvhdp_trees_current(self.h)
        if rc < 0:
            self._ck(rc)
        return bool(rc)

    def get_view_weights(self):
        p = np.empty((self.D, self.M, self.M), dtype=np.float64)
        self._ck(self.L.mvhdp_get_view_weights(self.h, _ptr(p)))
        return p

    # -- interop ----------------------------------------------------------------
    def device_buffer(self, which):
        ptr = C.c_void_p()
        nbytes = C.c_size_t()
        self._ck(self.L.mvhdp_device_buffer(self.h, int(which), C.byref(ptr), C.byref(nbytes)))
        return ptr.value, nbytes.value

    def counts_written(self):
        self._ck(self.L.mvhdp_counts_written(self.h))

    def set_stream(self, hip_stream):
        self._ck(self.L.mvhdp_set_stream(self.h, C.c_void_p(hip_stream) if hip_stream else None))

    def synchronize(self):
        self._ck(self.L.mvhdp_synchronize(self.h))


class NativeGroup:
    """Document shards on several GPUs, exchange step inside the library (include/mvhdp.h mvhdp_group_*): Python mirror of what
    the Java host of INTEGRATION.md calls.  Two ways to form one:

      NativeGroup(samplers)                            one process, one NativeSampler per GPU (or several on one GPU: tests)
      NativeGroup.from_rank(sampler, id, rank, n)      one process per GPU; `id` = NativeGroup.unique_id() of one rank, handed to
                                                       the others by the launcher (torch.distributed's store in bench.py)
    """

    def __init__(self, samplers=None, _handle=None, _members=None):
        self.L = load_library()
        if _handle is not None:
            self.g, self.members = _handle, list(_members)
            return
        self.members = list(samplers)
        arr = (C.c_void_p * len(self.members))(*[s.h for s in self.members])
        self.g = C.c_void_p()
        rc = self.L.mvhdp_group_create(len(self.members), arr, C.byref(self.g))
        if rc != 0:
            self.g = None
            raise MvhdpError(rc, self.L.mvhdp_group_last_error(None).decode())

    @staticmethod
    def unique_id():
        L = load_library()
        buf = (C.c_uint8 * UNIQUE_ID_BYTES)()
        rc = L.mvhdp_group_unique_id(C.cast(buf, C.c_void_p))
        if rc != 0:
            raise MvhdpError(rc, L.mvhdp_group_last_error(None).decode())
        return bytes(buf)

    @classmethod
    def from_rank(cls, sampler, unique_id, rank, nranks):
        L = load_library()
        assert len(unique_id) == UNIQUE_ID_BYTES
        buf = (C.c_uint8 * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        g = C.c_void_p()
        rc = L.mvhdp_group_create_rank(sampler.h, C.cast(buf, C.c_void_p), int(rank), int(nranks), C.byref(g))
        if rc != 0:
            raise MvhdpError(rc, L.mvhdp_group_last_error(None).decode())
        return cls(_handle=g, _members=[sampler])

    def _ck(self, rc):
        if rc != 0:
            raise MvhdpError(rc, self.L.mvhdp_group_last_error(self.g).decode())

    def close(self):
        if getattr(self, "g", None):
            self.L.mvhdp_group_destroy(self.g)
            self.g = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def info(self):
        t = GroupInfoC()
        self._ck(self.L.mvhdp_group_get_info(self.g, C.byref(t)))
        return t

    def set_exchange_chunks(self, n):
        self._ck(self.L.mvhdp_group_set_exchange_chunks(self.g, int(n)))

    def build_counts(self):
        self._ck(self.L.mvhdp_group_build_counts(self.g))

    def drain(self):
        """Lands the exchange a SWEEP_ASYNC_EXCHANGE sweep left on the wire: every replica is the global model again."""
        self._ck(self.L.mvhdp_group_drain(self.g))

    def abort(self):
        """This rank cannot go on: its next sweep contributes nothing and fails on every rank together."""
        self._ck(self.L.mvhdp_group_abort(self.g))

    # -- the steps either side of the sweep, for the sharded model (mvhdp_group_*: include/mvhdp.h) --
    def set_hyper(self, hy):
        for s in self.members:
            s.set_hyper(hy)                     # (keeps the arrays alive per member; same effect as mvhdp_group_set_hyper)

    def set_vectors_mix(self, lam, exp_dot=None, sum_exp=None):
        for s in self.members:                  # (every member carries its own copy of the table; the group checks that they agree)
            s.set_vectors_mix(lam, exp_dot, sum_exp)

    def remap_topics(self, topic_map, retire=False) -> RemapStats:
        """NativeSampler.remap_topics on every local member (every rank passes the same map); moved and dropped are summed over them.
        Refused unless the group is drained and not failed."""
        s0 = self.members[0]
        rc, st = _remap_call(self.L.mvhdp_group_remap_topics, self.g, s0.K, s0.M, topic_map, retire)
        self._ck(rc)
        return st

    def model_log_likelihood(self):
        M = self.members[0].M
        ll = np.zeros(M, dtype=np.float64)
        self._ck(self.L.mvhdp_group_log_likelihood(self.g, _ptr(ll)))
        return ll

    def get_doc_topic_hist(self, m, hist_len, len_len=0):
        hist = np.empty((self.members[0].K, hist_len), dtype=np.int32)
        dl = np.empty(max(len_len, 1), dtype=np.int32) if len_len > 0 else None
        self._ck(self.L.mvhdp_group_doc_topic_hist(self.g, m, _ptr(hist), hist_len, _ptr(dl), len_len))
        return hist, (dl[:len_len] if dl is not None else None)

    def get_count_histogram(self, m, length):
        h = np.zeros(length, dtype=np.int32)
        self._ck(self.L.mvhdp_group_count_histogram(self.g, m, _ptr(h), length))
        return h

    def view_overlap_sums(self):
        M = self.members[0].M
        s = np.zeros((M, M), dtype=np.float64)
        self._ck(self.L.mvhdp_group_view_overlap_sums(self.g, _ptr(s)))
        return s

    def gamma_doc_statistics(self, m, gamma_m, seed, round_idx):
        qs, qw = C.c_double(), C.c_double()
        self._ck(self.L.mvhdp_group_gamma_doc_statistics(self.g, int(m), float(gamma_m), int(seed), int(round_idx), C.byref(qs), C.byref(qw)))
        return qs.value, qw.value

    def diagnostics(self, num_top_words=20, vocabulary=None, word_length=None):
        """NativeSampler.diagnostics of the whole sharded model (mvhdp_group_diagnostics).  Top words and discrimination weights of a
        group are those of any member: NativeSampler.top_words / discr_weights on one of them."""
        s0 = self.members[0]
        rc, d = _run_diagnostics(self.L, self.L.mvhdp_group_diagnostics, self.g, s0.K, s0.V[0], s0.M, num_top_words, vocabulary, word_length)
        self._ck(rc)
        return d

    def topic_phrases(self, max_per_topic=20, vocabulary=None):
        """NativeSampler.topic_phrases of the sharded corpus, over the LOCAL members: every member's uncut lists merged
        (merge_topic_phrases).  A group of rank processes merges its ranks' results the same way on the host side."""
        r = merge_topic_phrases([s.topic_phrases(-1) for s in self.members], max_per_topic)
        if vocabulary is not None:
            r.phrases = [[(" ".join(str(vocabulary[i]) for i in ids), c) for ids, c in row] for row in r.phrases]
        return r

    def heldout_left_to_right(self, doc_off, tokens, particles=10, resample=True, seed=0, m=0, doc_base=0, alpha=None, alpha_sum=None,
                              want_position_sums=False):
        """NativeSampler.heldout_left_to_right with the held-out documents split over the LOCAL members in contiguous ranges of about equal
        sum of L^2 (the work of a document), each member told the global index of its first document.  Every member holds the whole
        counts and documents are independent, so every per-document value is the single handle's, bit for bit; the total adds them in
        document order on the host, as the library does."""
        doc_off, tokens = _heldout_docs(doc_off, tokens)
        D, n = len(doc_off) - 1, len(self.members)
        work = np.concatenate([[0.0], np.cumsum(np.diff(doc_off).astype(np.float64) ** 2)])
        cuts = [0] + [int(np.searchsorted(work, work[-1] * i / n, side="left")) for i in range(1, n)] + [D]
        cuts = [min(max(c, 0), D) for c in np.maximum.accumulate(cuts)]
        parts = []
        for s, d0, d1 in zip(self.members, cuts[:-1], cuts[1:]):
            t0, t1 = int(doc_off[d0]), int(doc_off[d1])
            parts.append(s.heldout_left_to_right(doc_off[d0:d1 + 1] - t0, tokens[t0:t1], particles, resample, seed, m, int(doc_base) + d0, alpha, alpha_sum,
                                                 want_position_sums))
        doc_ll = np.concatenate([p.doc_log_likelihood for p in parts])
        total = 0.0
        for x in doc_ll:
            total = total + float(x)
        return HeldoutResult(total, doc_ll, np.concatenate([p.position_sum for p in parts]) if want_position_sums else None,
                             np.concatenate([p.doc_tokens for p in parts]), sum(p.tokens for p in parts), sum(p.oov for p in parts),
                             sum(p.visits for p in parts), int(particles))

    def fold_in(self, doc_off, tokens, view_weights, iterations=10, samples=1, thin=1, seed=0, doc_base=0, coupling=None, want_z=False,
                want_counts=False):
        """NativeSampler.fold_in on the first LOCAL member, the group drained first: the model is replicated, so any member's answer is
        the group's."""
        if self.g is not None:
            self.drain()
        return self.members[0].fold_in(doc_off, tokens, view_weights, iterations, samples, thin, seed, doc_base, coupling, want_z, want_counts)

    def _member_ranges(self, d0, d1):
        """the LOCAL members' entities as one sequence, member after member: (member, first global id, local d0, local d1) of every
        member that holds a part of [d0, d1)"""
        bases = np.concatenate([[0], np.cumsum([s.D for s in self.members])]).astype(np.int64)
        d1 = int(bases[-1]) if d1 is None else int(d1)
        d0 = int(d0)
        if d0 < 0 or d1 > int(bases[-1]) or d0 > d1:
            raise ValueError("bad entity range")
        out = []
        for s, b, e in zip(self.members, bases[:-1], bases[1:]):
            lo, hi = max(d0, int(b)), min(d1, int(e))
            if lo < hi:
                out.append((s, int(b), lo - int(b), hi - int(b)))
        return out, d0, d1

    def word_cooccurrence(self, sets, m=0, window=0, d0=0, d1=None, corpus=None) -> WordCooccurrence:
        """NativeSampler.word_cooccurrence of the sharded corpus, over the LOCAL members: every member counts its own entities of
        [d0, d1) (entity ids count through the members in their order) and the parts are summed (merge_word_cooccurrence): exact, because
        a window never crosses an entity.  A caller's corpus is no member's: the first member counts it.  A group of rank processes merges
        its ranks' results the same way on the host side."""
        if corpus is not None:
            return self.members[0].word_cooccurrence(sets, m, window, d0, d1, corpus)
        parts, d0, d1 = self._member_ranges(d0, d1)
        if not parts:                                                        # an empty range: the first member answers with its zeros
            return self.members[0].word_cooccurrence(sets, m, window, 0, 0)
        return merge_word_cooccurrence([s.word_cooccurrence(sets, m, window, lo, hi) for s, _, lo, hi in parts])

    def predict_items(self, m, view_weights, n, d0=0, d1=None, exclude_present=True, theta=None):
        """NativeSampler.predict_items over the LOCAL members: the counts are replicated and the entities partitioned, so every member
        answers for its own entities and the rows are concatenated in entity order (entity ids count through the members in their
        order); per entity the values are a single handle's, bit for bit.  (As with doc_topic_proportions on a shard, the carry-over of
        a missing view does not reach across a member's first entity.)"""
        parts, d0, d1 = self._member_ranges(d0, d1)
        th = None if theta is None else np.ascontiguousarray(theta, dtype=np.float64)
        got = [s.predict_items(m, view_weights, n, lo, hi, exclude_present, None if th is None else th[b + lo - d0:b + hi - d0]) for s, b, lo, hi in parts]
        if not got:
            return np.full((0, int(n)), -1, dtype=np.int32), np.zeros((0, int(n))), np.zeros(0, dtype=np.int32)
        return tuple(np.concatenate([g[i] for g in got]) for i in range(3))

    def score_items(self, m, view_weights, entities, items, d0=0, d1=None, exclude_present=True, theta=None):
        """NativeSampler.score_items over the LOCAL members: every pair goes to the member that holds its entity; the results come back
        in the order of the pairs."""
        parts, d0, d1 = self._member_ranges(d0, d1)
        ent = np.ascontiguousarray(entities, dtype=np.int64)
        it = np.ascontiguousarray(items, dtype=np.int32)
        if ent.ndim != 1 or ent.shape != it.shape:
            raise ValueError("entities and items: two arrays of one length")
        if len(ent) and (ent.min() < d0 or ent.max() >= d1):
            raise ValueError("an entity outside [d0, d1)")
        th = None if theta is None else np.ascontiguousarray(theta, dtype=np.float64)
        score = np.zeros(len(ent), dtype=np.float64)
        rank = np.zeros(len(ent), dtype=np.int32)
        for s, b, lo, hi in parts:
            at = np.flatnonzero((ent >= b + lo) & (ent < b + hi))
            if len(at) == 0:
                continue
            r = s.score_items(m, view_weights, ent[at] - b, it[at], lo, hi, exclude_present, None if th is None else th[b + lo - d0:b + hi - d0])
            score[at], rank[at] = r.score, r.rank
        return ItemScores(score, rank)

    def nearest_entities(self, view_weights, n, queries, min_weight=-np.inf, **knobs):
        """NativeSampler.nearest_entities for host-row queries over the LOCAL members: every member answers for its own entities, its
        ids are moved to the group's numbering (entity ids count through the members in their order) and the lists are merged
        (merge_nearest): per pair the values are a single handle's, bit for bit.  (As with doc_topic_proportions on a shard, the
        carry-over of a missing view does not reach across a member's first entity.)"""
        bases = np.concatenate([[0], np.cumsum([s.D for s in self.members])]).astype(np.int64)
        parts = []
        for s, b in zip(self.members, bases[:-1]):
            r = s.nearest_entities(view_weights, n, queries=queries, min_weight=min_weight, **knobs)
            r.ids[r.ids >= 0] += int(b)
            parts.append(r)
        return merge_nearest(parts, n)

    def predict_entities(self, m, view_weights, n, items=None, weights=None, psi=None, exclude_present=True, **knobs):
        """NativeSampler.predict_entities over the LOCAL members: the counts are replicated, so every member builds the same psi and
        answers for its own entities; its ids are moved to the group's numbering (entity ids count through the members in their
        order) and the lists are merged (merge_predicted_entities): per (entity, query) the values are a single handle's, bit for
        bit.  (The carry-over of a missing view does not reach across a member's first entity.)"""
        bases = np.concatenate([[0], np.cumsum([s.D for s in self.members])]).astype(np.int64)
        parts = []
        for s, b in zip(self.members, bases[:-1]):
            r = s.predict_entities(m, view_weights, n, items=items, weights=weights, psi=psi, exclude_present=exclude_present, **knobs)
            r.ids[r.ids >= 0] += int(b)
            parts.append(r)
        return merge_predicted_entities(parts, n)

    def topic_top_entities(self, view_weights, n, threshold=-np.inf, **knobs):
        """NativeSampler.topic_top_entities over the LOCAL members' entities, merged the same way (merge_topic_top_entities)."""
        bases = np.concatenate([[0], np.cumsum([s.D for s in self.members])]).astype(np.int64)
        parts = []
        for s, b in zip(self.members, bases[:-1]):
            ids, weights, counts = s.topic_top_entities(view_weights, n, threshold, **knobs)
            ids[ids >= 0] += int(b)
            parts.append((ids, weights, counts))
        return merge_topic_top_entities(parts, n)

    def topic_gram(self, source, m=0, view_weights=None, transform="identity", threshold=None, blocks_per_pass=0):
        """NativeSampler.topic_gram over the LOCAL members.  "words" and host rows go to the first member: the counts are replicated.
        "entities" runs on every member over its own entities and the results are merged in member order (merge_topic_grams): the
        integers n_above and co_above equal a single handle's; gram and sums are the member-order sum of the members' results, NOT a
        single handle's bits.  (The carry-over of a missing view does not reach across a member's first entity.)"""
        if not (isinstance(source, str) and source == "entities"):
            return self.members[0].topic_gram(source, m=m, view_weights=view_weights, transform=transform, threshold=threshold, blocks_per_pass=blocks_per_pass)
        return merge_topic_grams([s.topic_gram("entities", view_weights=view_weights, transform=transform, threshold=threshold, blocks_per_pass=blocks_per_pass)
                                  for s in self.members])

    def sweep(self, sweep_idx, seed, flags=0):
        """One sweep of the whole model; the list of the local members' statistics."""
        n = len(self.members)
        arr = (SweepStatsC * n)()
        self._ck(self.L.mvhdp_group_sweep(self.g, int(sweep_idx), int(seed), int(flags), C.cast(arr, C.c_void_p)))
        return [SweepStats(**{f: getattr(arr[i], f) for f, _ in SweepStatsC._fields_}) for i in range(n)]
