"""The topic diagnostics restated in numpy: the checker of mvhdp_top_words / mvhdp_discr_weights / mvhdp_diagnostics.

Restates, from the reference's own lines (aliases as in include/mvhdp.h; DIAG = FastQMVWVTopicModelDiagnostics.java):
  getSortedWords                         PTM:1792-1811  (TreeSet<IDSorter>: count descending, equal counts by descending type id)
  calcDiscrWeightAcrossTopicsPerModality PTM:2181-2230  (skewSum / nonZeroSkewCnt carried across views, the count starting at 1)
  calcDiscrWeightWithinTopics            PTM:2233-2270
  the constructor and collectDocumentStatistics DIAG:53-236, the score rows DIAG:242-612.
Every floating-point sum runs in the reference's order (TreeSet order, document order, ascending topics) with IEEE float64
operations in the reference's expression order; scalar logarithms go through the math module.  Test infrastructure only: imports
nothing from the product.
"""
import math

import numpy as np

DEFAULT_DOC_PROPORTIONS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)      # DIAG:27
TWO_PERCENT_INDEX, FIFTY_PERCENT_INDEX = 1, 6                          # DIAG:25-26
ROWS = ["tokens", "document_entropy", "word-length", "coherence", "normDiscrWeight", "discrWeight", "uniform_dist",
        "corpus_dist", "eff_num_words", "token-doc-diff", "rank_1_docs", "allocation_ratio", "allocation_count"]


class JavaArithmeticError(Exception):
    """What the reference's pass would throw (an unassigned or out-of-vocabulary view-0 token, DIAG:171-173)."""


def _seq_sum(a):
    """a[0] + a[1] + ... left to right (np.cumsum is a sequential loop)."""
    a = np.asarray(a, dtype=np.float64)
    return float(np.cumsum(a)[-1]) if a.size else 0.0


def jdiv(a, b):
    """Java double division, including x / 0."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def jlog(x):
    if x > 0:
        return math.log(x)
    if x == 0:
        return -math.inf
    return math.nan


def jlog10(x):
    if x > 0:
        return math.log10(x)
    if x == 0:
        return -math.inf
    return math.nan


def sorted_words(nwk):
    """getSortedWords PTM:1792-1811: per topic, [(type, count)] in TreeSet<IDSorter> order."""
    nwk = np.asarray(nwk)
    out = []
    for k in range(nwk.shape[1]):
        col = nwk[:, k]
        types = np.nonzero(col > 0)[0]
        counts = col[types]
        order = np.lexsort((-types, -counts.astype(np.int64)))
        out.append((types[order].astype(np.int64), counts[order].astype(np.int64)))
    return out


def top_words(nwk, n):
    """(types [K][n] with -1 unfilled, counts [K][n] with 0 unfilled, nonzero [K])."""
    sw = sorted_words(nwk)
    K = len(sw)
    t = np.full((K, n), -1, np.int32)
    c = np.zeros((K, n), np.int32)
    nz = np.zeros(K, np.int32)
    for k, (ty, cn) in enumerate(sw):
        r = min(n, len(ty))
        t[k, :r] = ty[:r]
        c[k, :r] = cn[:r]
        nz[k] = len(ty)
    return t, c, nz


def type_discr_weight(nwk):
    """typeDiscrWeight[m][type] PTM:2196-2215: sum_k pow(c, 2) (a double sum over ascending topics) / pow(total, 2), 0 for an empty row."""
    nwk = np.asarray(nwk, dtype=np.int64)
    sq = np.cumsum((nwk * nwk).astype(np.float64), axis=1)[:, -1] if nwk.shape[1] else np.zeros(nwk.shape[0])
    tot = nwk.sum(axis=1)
    out = np.zeros(nwk.shape[0])
    pos = tot > 0
    out[pos] = sq[pos] / (tot[pos].astype(np.float64) * tot[pos].astype(np.float64))
    return out


def discr_weight_per_view(nwk_views):
    """calcDiscrWeightAcrossTopicsPerModality PTM:2181-2230 (accumulators not reset between views, nonZeroSkewCnt from 1)."""
    skewSum = 0.0
    nonZeroSkewCnt = 1
    out = []
    for nwk in nwk_views:
        tw = type_discr_weight(nwk)
        for x in tw[tw > 0]:                          # type order
            skewSum += float(x)
            nonZeroSkewCnt += 1
        out.append(skewSum / nonZeroSkewCnt)
    return np.array(out)


def discr_weight_within_topics(sw, tw):
    """calcDiscrWeightWithinTopics(.., true, 0) PTM:2243-2267 over the TreeSets of view 0."""
    out = np.zeros(len(sw))
    for k, (ty, cn) in enumerate(sw):
        w = tw[ty] * cn.astype(np.float64)            # tokenWeight * info.getWeight()
        total = _seq_sum(w)
        with np.errstate(divide="ignore", invalid="ignore"):
            p = w / total
        out[k] = _seq_sum(p * p)
    return out


def document_statistics(doc_off, tokens, z, K, V0, top_types, nonzero, N, gamma0, alpha0, alpha_sum0):
    """collectDocumentStatistics DIAG:120-236 over the view-0 entities (vectorised; sums in document order per topic).
    top_types: [K][N] with -1 unfilled (the reference's int[] holds 0 there, DIAG:132: the padding quirk)."""
    doc_off = np.asarray(doc_off, dtype=np.int64)
    tokens = np.asarray(tokens, dtype=np.int64)
    z = np.asarray(z, dtype=np.int64)
    D = len(doc_off) - 1
    if tokens.size and (z.min() < 0 or z.max() >= K or tokens.min() < 0 or tokens.max() >= V0):
        raise JavaArithmeticError("unassigned or out-of-vocabulary view-0 token")
    lens = np.diff(doc_off)
    doc_of_tok = np.repeat(np.arange(D, dtype=np.int64), lens)
    word_type_counts = np.bincount(tokens, minlength=V0).astype(np.int64)          # DIAG:171
    num_tokens = int(tokens.size)                                                   # DIAG:170
    # the top-N positions of each topic's real top words (DIAG:146-152)
    nreal = np.minimum(nonzero, N)
    pos_of = {}
    lut = np.full((K, V0), -1, np.int8) if K * V0 <= 400_000_000 else None
    for k in range(K):
        for i in range(nreal[k]):
            if lut is not None:
                lut[k, top_types[k, i]] = i
            else:
                pos_of[(k, int(top_types[k, i]))] = i
    if lut is not None:
        tpos = lut[z, tokens].astype(np.int64)
    else:
        tpos = np.array([pos_of.get((int(a), int(b)), -1) for a, b in zip(z, tokens)], dtype=np.int64)
    tbit = np.where(tpos >= 0, np.left_shift(np.uint64(1), np.maximum(tpos, 0).astype(np.uint64)), np.uint64(0)).astype(np.uint64)
    # (doc, topic) pairs in document order, ascending topics
    key = doc_of_tok * K + z
    order = np.argsort(key, kind="stable")
    ks = key[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]]) if ks.size else np.zeros(0, np.int64)
    pair_key = ks[starts]
    pair_cnt = np.diff(np.r_[starts, ks.size]).astype(np.int64)
    pair_mask = np.bitwise_or.reduceat(tbit[order], starts) if ks.size else np.zeros(0, np.uint64)
    pair_doc = pair_key // K
    pair_topic = pair_key % K
    pair_len = lens[pair_doc]
    num_nonzero = np.bincount(pair_topic, minlength=K).astype(np.int64)             # DIAG:189
    # sumCountTimesLogCount DIAG:196: per topic, in document order
    clc = pair_cnt.astype(np.float64) * np.array([math.log(c) for c in pair_cnt], dtype=np.float64) if pair_cnt.size < 2_000_000 \
        else pair_cnt.astype(np.float64) * np.log(pair_cnt.astype(np.float64))
    by_topic = np.argsort(pair_topic, kind="stable")
    tstarts = np.searchsorted(pair_topic[by_topic], np.arange(K))
    tends = np.searchsorted(pair_topic[by_topic], np.arange(K), side="right")
    sclc = np.array([_seq_sum(clc[by_topic[a:b]]) for a, b in zip(tstarts, tends)])
    # proportions DIAG:198-204: (gamma0 * alpha0[k] + c) / ((double) gamma0 * alphaSum0 + docLength)
    prop = (gamma0 * np.asarray(alpha0, dtype=np.float64)[pair_topic] + pair_cnt.astype(np.float64)) / \
           (np.float64(gamma0) * np.float64(alpha_sum0) + pair_len.astype(np.float64))
    at_prop = np.zeros((K, len(DEFAULT_DOC_PROPORTIONS)), np.int64)
    reach = np.ones(prop.shape, bool)
    for i, th in enumerate(DEFAULT_DOC_PROPORTIONS):
        reach &= ~(prop < th)                                                       # `if (proportion < p) break;`
        at_prop[:, i] = np.bincount(pair_topic[reach], minlength=K)
    # rank 1 DIAG:183-194,228-230: the largest count, the lowest topic among equals
    r1 = np.lexsort((pair_topic, -pair_cnt, pair_doc))
    first = np.r_[True, pair_doc[r1][1:] != pair_doc[r1][:-1]] if r1.size else np.zeros(0, bool)
    num_rank1 = np.bincount(pair_topic[r1][first], minlength=K).astype(np.int64)
    # co-document matrices DIAG:206-221 with the padding quirk: an unfilled position holds type 0
    allN = np.uint64((1 << N) - 1) if N < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    pos0 = np.full(K, -1, np.int64)
    for k in range(K):
        for i in range(nreal[k]):
            if top_types[k, i] == 0:
                pos0[k] = i
    pm = pair_mask.copy()
    nr_p = nreal[pair_topic].astype(np.int64)
    p0_p = pos0[pair_topic]
    pad = (nr_p < N) & (p0_p >= 0)
    if pad.any():
        has0 = np.zeros(pm.shape, bool)
        has0[pad] = ((pm[pad] >> p0_p[pad].astype(np.uint64)) & np.uint64(1)) == np.uint64(1)
        low = np.array([(1 << int(r)) - 1 for r in nr_p[has0]], dtype=np.uint64)
        pm[has0] |= allN & ~low
    codoc = np.zeros((K, N, N), np.int64)
    sel = pm != 0
    if sel.any():
        if N + int(K).bit_length() <= 64:                     # one sortable key per (topic, mask)
            uk, mult = np.unique((pair_topic[sel].astype(np.uint64) << np.uint64(N)) | pm[sel], return_counts=True)
            tk, mk = (uk >> np.uint64(N)).astype(np.int64), uk & allN
        else:
            uk, mult = np.unique(np.stack([pair_topic[sel].astype(np.uint64), pm[sel]]), axis=1, return_counts=True)
            tk, mk = uk[0].astype(np.int64), uk[1]
        bits = [((mk >> np.uint64(i)) & np.uint64(1)).astype(bool) for i in range(N)]
        for i in range(N):
            if not bits[i].any():
                continue
            codoc[:, i, i] += np.bincount(tk[bits[i]], weights=mult[bits[i]], minlength=K).astype(np.int64)
            for j in range(i + 1, N):
                both = bits[i] & bits[j]
                if both.any():
                    c = np.bincount(tk[both], weights=mult[both], minlength=K).astype(np.int64)
                    codoc[:, i, j] += c
                    codoc[:, j, i] += c
    return dict(word_type_counts=word_type_counts, num_tokens=num_tokens, num_nonzero_docs=num_nonzero,
                sum_count_log_count=sclc, num_docs_at_proportions=at_prop, num_rank1_docs=num_rank1, codoc=codoc)


def diagnostics(nwk_views, nk0, alpha, gamma0, alpha_sum0, beta0, doc_off0, tokens0, z0, N, word_length=None):
    """FastQMVWVTopicModelDiagnostics(model, N) DIAG:53-117.  nwk_views: n_wk [V_m][K] of every view; nk0: tokensPerTopic[0];
    alpha: alpha[0][0..K] (K+1 entries).  Returns the scores / word scores by row name and the accumulators."""
    nwk0 = np.asarray(nwk_views[0])
    V0, K = nwk0.shape
    sw = sorted_words(nwk0)
    top_t, top_c, nonzero = top_words(nwk0, N)
    ds = document_statistics(doc_off0, tokens0, z0, K, V0, top_t, nonzero, N, gamma0, np.asarray(alpha)[:K], alpha_sum0)
    per_view = discr_weight_per_view(nwk_views)
    tw0 = type_discr_weight(nwk0)
    tdw = discr_weight_within_topics(sw, tw0)
    alpha = np.asarray(alpha, dtype=np.float64)
    sc = {r: np.zeros(K) for r in ROWS}
    ws = {r: np.zeros((K, N)) for r in ROWS}
    numTokens = ds["num_tokens"]
    wtc = ds["word_type_counts"]
    codoc = ds["codoc"]
    avgAlpha, cnt = 0.0, 0                                                          # DIAG:315-325
    for kk in range(K + 1):
        avgAlpha += float(alpha[kk])
        cnt += 0 if alpha[kk] == 0 else 1
    avgAlpha = jdiv(avgAlpha, cnt)
    for k in range(K):
        T = int(nk0[k])
        ty, cn = sw[k]
        nr = min(N, len(ty))
        sc["tokens"][k] = T                                                         # DIAG:242-250
        sc["document_entropy"][k] = jdiv(-ds["sum_count_log_count"][k], T) + jlog(T)   # DIAG:256
        if word_length is None:
            sc["word-length"][k] = math.nan
            ws["word-length"][k, :] = math.nan
        else:                                                                       # DIAG:462-483
            total = 0
            for i in range(nr):
                L = int(word_length[ty[i]])
                total += L
                ws["word-length"][k, i] = L
            sc["word-length"][k] = total / N
        m = codoc[k]
        topicScore = 0.0                                                            # DIAG:544-570
        for row in range(N):
            rowScore, minScore = 0.0, 0.0
            for col in range(row):
                score = jlog(jdiv(m[row, col] + beta0, m[col, col] + beta0))
                rowScore += score
                if score < minScore:
                    minScore = score
            topicScore += rowScore
            ws["coherence"][k, row] = minScore
        sc["coherence"][k] = topicScore
        if alpha[k] != 0:                                                           # DIAG:297-338
            diffLogWeight = abs(jlog10(alpha[k]) - jlog10(avgAlpha))
            sc["normDiscrWeight"][k] = jdiv(tdw[k], diffLogWeight)
            sc["discrWeight"][k] = tdw[k]
        # uniform_dist DIAG:262-295, corpus_dist DIAG:368-404, eff_num_words DIAG:340-363: TreeSet order
        coefficient = jdiv(numTokens, T)
        tu = tc = se = 0.0
        for pos in range(len(ty)):
            count = float(cn[pos])
            s_u = jdiv(count, T) * jlog(jdiv(count * V0, T))
            s_c = jdiv(count, T) * jlog(jdiv(coefficient * count, wtc[ty[pos]]))
            p = jdiv(count, T)
            if pos < N:
                ws["uniform_dist"][k, pos] = s_u
                ws["corpus_dist"][k, pos] = s_c
            tu += s_u
            tc += s_c
            se += p * p
        sc["uniform_dist"][k] = tu
        sc["corpus_dist"][k] = tc
        sc["eff_num_words"][k] = jdiv(1.0, se)
        wd = np.zeros(N)                                                            # DIAG:406-457
        dd = np.zeros(N)
        wordSum = docSum = 0.0
        for pos in range(nr):
            wd[pos] = cn[pos]
            dd[pos] = m[pos, pos]
            wordSum += wd[pos]
            docSum += dd[pos]
        ts = 0.0
        for pos in range(N):
            p = jdiv(wd[pos], wordSum)
            q = jdiv(dd[pos], docSum)
            meanProb = 0.5 * (p + q)
            score = 0.0
            if p > 0:
                score += 0.5 * p * jlog(jdiv(p, meanProb))
            if q > 0:
                score += 0.5 * q * jlog(jdiv(q, meanProb))
            ws["token-doc-diff"][k, pos] = score
            ts += score
        sc["token-doc-diff"][k] = ts
        nzd = int(ds["num_nonzero_docs"][k])
        ap = ds["num_docs_at_proportions"][k]
        sc["rank_1_docs"][k] = jdiv(int(ds["num_rank1_docs"][k]), nzd)               # DIAG:573-581
        sc["allocation_ratio"][k] = jdiv(int(ap[FIFTY_PERCENT_INDEX]), int(ap[TWO_PERCENT_INDEX]))   # DIAG:583-598
        sc["allocation_count"][k] = jdiv(int(ap[5]), nzd)                           # DIAG:600-613
    out = dict(ds)
    out.update(scores=sc, word_scores=ws, top_types=top_t, top_counts=top_c, nonzero=nonzero, discr_weight_per_view=per_view,
               type_discr_weight0=tw0, discr_weight_within=tdw)
    return out


def uniform_abs_sum(nwk0, nk0):
    """sum over every (word, topic) of |uniform_dist term|: the scale of the signed sum's rounding (per topic)."""
    nwk0 = np.asarray(nwk0, dtype=np.float64)
    V0 = nwk0.shape[0]
    T = np.asarray(nk0, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(nwk0 > 0, (nwk0 / T) * np.log((nwk0 * V0) / T), 0.0)
    return np.abs(t).sum(axis=0)


def corpus_abs_sum(nwk0, nk0, word_type_counts, num_tokens):
    nwk0 = np.asarray(nwk0, dtype=np.float64)
    T = np.asarray(nk0, dtype=np.float64)
    wtc = np.asarray(word_type_counts, dtype=np.float64)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(nwk0 > 0, (nwk0 / T) * np.log((num_tokens / T) * nwk0 / wtc), 0.0)
    return np.abs(t).sum(axis=0)
