"""TEST INFRASTRUCTURE ONLY: numpy restatement of mvhdp_nearest_entities, mvhdp_topic_top_entities and native.merge_nearest
(include/mvhdp.h), built on tests/sim_numpy.py: clean and norms are that module's, the k-ordered chain is the same one for a rectangular
pair of matrices.  numpy's elementwise +, *, / and sqrt on float64 are IEEE operations without fusion, so the bits are the contract's.
The geometry functions restate mvtopicmodel_amd/csrc/mvhdp_nearest.h for mvhdp_nearest_probe."""
import numpy as np

from tests import sim_numpy as sn

TILE, MAX_STRIPE, AUTO_BLOCK, SCORE_CELLS = 128, 8192, 8192, 1 << 26
margin = sn.margin


def dots_rect(q, x):
    """[nq][nc]: s = s + q_k * x_k over ascending k from +0.0, product and sum rounded separately"""
    acc = np.zeros((q.shape[0], x.shape[0]))
    with np.errstate(all="ignore"):
        for k in range(q.shape[1]):
            acc = acc + np.outer(q[:, k], x[:, k])
    return acc


def cosine_rect(queries, cands, min_weight=-np.inf):
    """(sim [nq][nc], query may list [nq], candidate may be listed [nc]): MVHDP_SIM_COS of mvhdp_similar_pairs for every pair"""
    q, x = sn.clean(queries, min_weight), sn.clean(cands, min_weight)
    nq, nx = sn.norms(q), sn.norms(x)
    with np.errstate(all="ignore"):
        sim = dots_rect(q, x) / (nq[:, None] * nx[None, :])
    return sim, (nq > 0) & np.isfinite(nq), (nx > 0) & np.isfinite(nx)


def first_n(values, ids, n):
    """positions of the first n by (value descending, id ascending); a NaN value is never listed"""
    keep = np.flatnonzero(~np.isnan(values))
    return keep[np.lexsort((ids[keep], -values[keep]))][:n]


def nearest(queries, cands, n, min_weight=-np.inf, self_index=None, id_base=0, matrix=None):
    """(ids [nq][n] (-1), sims [nq][n] (0.0), counts [nq]).  self_index [nq]: the candidate row that is query q itself and is left out
    (-1: none), or None.  ids are id_base + the candidate's row.  matrix: a cosine_rect() result to reuse."""
    sim, okq, okc = cosine_rect(queries, cands, min_weight) if matrix is None else matrix
    nq, nc = sim.shape
    ids = np.full((nq, n), -1, dtype=np.int64)
    sims = np.zeros((nq, n))
    counts = np.zeros(nq, dtype=np.int32)
    col = np.arange(nc, dtype=np.int64)
    for q in range(nq):
        if not okq[q]:
            continue
        may = okc.copy()
        if self_index is not None and 0 <= self_index[q] < nc:
            may[self_index[q]] = False
        at = np.flatnonzero(may)
        o = at[first_n(sim[q, at], col[at], n)]
        counts[q] = len(o)
        ids[q, :len(o)], sims[q, :len(o)] = id_base + o, sim[q, o]
    return ids, sims, counts


def topic_top_entities(prop, n, threshold=-np.inf, id_base=0):
    """(ids [K][n] (-1), weights [K][n] (0.0), counts [K]): per topic the entities with prop > threshold, weight descending, id ascending"""
    D, K = prop.shape
    ids = np.full((K, n), -1, dtype=np.int64)
    weights = np.zeros((K, n))
    counts = np.zeros(K, dtype=np.int32)
    d = np.arange(D, dtype=np.int64)
    for k in range(K):
        at = np.flatnonzero(prop[:, k] > threshold)
        o = at[first_n(prop[at, k], d[at], n)]
        counts[k] = len(o)
        ids[k, :len(o)], weights[k, :len(o)] = id_base + o, prop[o, k]
    return ids, weights, counts


def merge(parts, n):
    """per row the first n of the listed entries of all parts: parts are (ids, values, counts) triples in one id numbering"""
    rows = len(parts[0][2])
    ids = np.full((rows, n), -1, dtype=np.int64)
    vals = np.zeros((rows, n))
    counts = np.zeros(rows, dtype=np.int32)
    for r in range(rows):
        i = np.concatenate([p[0][r, :p[2][r]] for p in parts])
        v = np.concatenate([p[1][r, :p[2][r]] for p in parts])
        o = first_n(v, i, n)
        counts[r] = len(o)
        ids[r, :len(o)], vals[r, :len(o)] = i[o], v[o]
    return ids, vals, counts


def screen_f32_rect(queries, cands):
    """[nq][nc] the screen's arithmetic: rows normalised in fp64, stored as fp32, one fp32 fma chain over ascending k (the product of two
    fp32 values is exact in fp64; rounding the fp64 sum to fp32 again moves a result by at most 2^-53 of it)"""
    q, x = np.asarray(queries, np.float64), np.asarray(cands, np.float64)
    fq = (q / sn.norms(q)[:, None]).astype(np.float32).astype(np.float64)
    fx = (x / sn.norms(x)[:, None]).astype(np.float32).astype(np.float64)
    s = np.zeros((q.shape[0], x.shape[0]), np.float32)
    for k in range(q.shape[1]):
        s = (np.outer(fq[:, k], fx[:, k]) + s.astype(np.float64)).astype(np.float32)
    return s.astype(np.float64)


# ---- the geometry of mvhdp_nearest.h ----
def stripe(stripe_candidates):
    return stripe_candidates if 0 < stripe_candidates < MAX_STRIPE else MAX_STRIPE


def block(block_queries, stripe_candidates):
    return min(block_queries if block_queries > 0 else AUTO_BLOCK, SCORE_CELLS // stripe(stripe_candidates))


def tiles(rows):
    return (rows + TILE - 1) // TILE


def blocks(nq, nc, block_queries=0, stripe_candidates=0):
    B = block(block_queries, stripe_candidates)
    return 0 if nq < 1 or nc < 1 else (nq + B - 1) // B


def cells(nq, nc, block_queries=0, stripe_candidates=0):
    if nq < 1 or nc < 1:
        return 0
    B, S = block(block_queries, stripe_candidates), stripe(stripe_candidates)
    total = 0
    for q0 in range(0, nq, B):
        for s0 in range(0, nc, S):
            total += tiles(min(q0 + B, nq) - q0) * tiles(min(s0 + S, nc) - s0) * TILE * TILE
    return total
