"""TEST INFRASTRUCTURE ONLY: numpy restatement of mvhdp_similar_pairs, mvhdp_doc_topics_top and mvhdp_entity_topic_distributions
(include/mvhdp.h).  Vectorised over the pairs, but every value goes through the reference's operations in the reference's order
(mallet-2.0.8 class files; FLOW = SciTopicFlow.java, PTM = FastQMVWVParallelTopicModel.java):
  dot   SparseVector.dotProductInternal / MatrixOps.dotProduct: s = s + a_k * b_k over ascending k, product and sum rounded separately
  norm  SparseVector.twoNorm / MatrixOps.twoNorm: Math.sqrt of the same chain of squares
  cos   dot / (|a| * |b|); folded: 1 - |1 - cos| (FLOW:1483)
  jsd   Maths.jensenShannonDivergence with math.log per term
numpy's elementwise +, *, / and sqrt on float64 are IEEE operations without fusion, so the bits are Java's."""
import math

import numpy as np

COS_FOLDED, COS, JSD = 0, 1, 2
_log = np.frompyfunc(math.log, 1, 1)


def margin(dim):
    return (dim + 4) * 2.0 ** -23


def clean(x, min_weight=-np.inf):
    x = np.array(x, dtype=np.float64)
    x[x <= min_weight] = 0.0
    return x


def norms(x):
    s = np.zeros(x.shape[0])
    with np.errstate(all="ignore"):
        for k in range(x.shape[1]):
            s = s + x[:, k] * x[:, k]
        return np.sqrt(s)


def dots(x):
    acc = np.zeros((x.shape[0], x.shape[0]))
    with np.errstate(all="ignore"):
        for k in range(x.shape[1]):
            acc = acc + np.outer(x[:, k], x[:, k])
    return acc


def cosine_matrix(x, metric):
    na = norms(x)
    with np.errstate(all="ignore"):
        c = dots(x) / (na[:, None] * na[None, :])
        if metric == COS_FOLDED:
            c = 1.0 - np.abs(1.0 - c)
    return c, na


def jsd_matrix(x):
    """[n][n]: klDivergence skips p_k == 0, returns +inf where p_k != 0 and m_k == 0, divides the sum by Math.log(2)."""
    n, dim = x.shape
    klp = np.zeros((n, n))          # KL(row i, m_ij)
    klq = np.zeros((n, n))          # KL(row j, m_ij)
    infp = np.zeros((n, n), bool)
    infq = np.zeros((n, n), bool)
    with np.errstate(all="ignore"):
        for k in range(dim):
            col = x[:, k]
            if not col.any():
                continue
            p = np.broadcast_to(col[:, None], (n, n))
            q = np.broadcast_to(col[None, :], (n, n))
            m = 0.0 + (p + q) / 2.0
            for v, kl, inf in ((p, klp, infp), (q, klq, infq)):
                on = v != 0.0
                inf |= on & (m == 0.0)
                go = on & (m != 0.0)
                if go.any():
                    kl[go] = kl[go] + v[go] * _log(v[go] / m[go]).astype(np.float64)
        ln2 = math.log(2.0)
        a = np.where(infp, np.inf, klp / ln2)
        b = np.where(infq, np.inf, klq / ln2)
        return (a + b) / 2.0


def sim_matrix(x, metric, min_weight=-np.inf):
    """(sim [n][n], can_pair [n]): rows whose norm is 0, Inf or NaN never pair."""
    x = clean(x, min_weight)
    if metric == JSD:
        na = norms(x)
        s = jsd_matrix(x)
    else:
        s, na = cosine_matrix(x, metric)
    return s, (na > 0) & np.isfinite(na)


def similar_pairs(x, metric, threshold, min_weight=-np.inf, matrix=None):
    """(i, j, sim) of all pairs i < j with sim > threshold, sorted by (i, j).  matrix: a sim_matrix() result to reuse."""
    s, ok = sim_matrix(x, metric, min_weight) if matrix is None else matrix
    with np.errstate(invalid="ignore"):
        hit = np.triu(s > threshold, 1) & ok[:, None] & ok[None, :]
    i, j = np.nonzero(hit)
    return i.astype(np.int32), j.astype(np.int32), s[i, j]


def screen_f32(a, b):
    """The screen's arithmetic for one pair of rows: normalised in fp64, stored as fp32, one fp32 fma chain (a_k * b_k is exact in fp64;
    the second rounding of the sum, fp64 then fp32, moves a result by at most 2^-53 of it)."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    na, nb = norms(a[None, :])[0], norms(b[None, :])[0]
    fa, fb = (a / na).astype(np.float32), (b / nb).astype(np.float32)
    s = np.float32(0.0)
    for k in range(len(fa)):
        s = np.float32(np.float64(fa[k]) * np.float64(fb[k]) + np.float64(s))
    return float(s)


def doc_topics_top(prop, threshold, max_topics):
    """PTM:2890-2926 on a [D][K] proportions matrix: (row_off, topics, weights).  IDSorter.compareTo: weight descending, equal weights by
    DESCENDING topic id."""
    D, K = prop.shape
    if max_topics < 0 or max_topics > K:
        max_topics = K
    off, topics, weights = [0], [], []
    for d in range(D):
        order = sorted(range(K), key=lambda k: (-prop[d, k], -k))
        for i in range(max_topics):
            k = order[i]
            if prop[d, k] < threshold:
                break
            topics.append(k)
            weights.append(prop[d, k])
        off.append(len(topics))
    return np.array(off, np.int64), np.array(topics, np.int32), np.array(weights, np.float64)


def round_half_up(v, digits):
    scale = 1.0
    for _ in range(digits):
        scale = scale * 10.0
    return np.floor(np.asarray(v, np.float64) * scale + 0.5) / scale


def entity_topic_distributions(prop, threshold, max_topics, round_digits, groups):
    """include/mvhdp.h: per group the kept weights, each floor(w * 10^4 + 0.5) / 10^4, summed per topic over the members in order; the
    total one chain over the members in order and ascending topic; sum / total, rounded to round_digits (-1: not)."""
    D, K = prop.shape
    off, topics, weights = doc_topics_top(prop, threshold, max_topics)
    out = np.zeros((len(groups), K))
    for g, members in enumerate(groups):
        s = np.zeros(K)
        total = 0.0
        for d in members:
            kept = sorted((int(topics[e]), float(round_half_up(weights[e], 4))) for e in range(off[d], off[d + 1]))
            for k, w in kept:
                s[k] = s[k] + w
                total = total + w
        if total != 0.0:
            v = s / total
            out[g] = v if round_digits < 0 else round_half_up(v, round_digits)
    return out
