"""Topic maps for NativeSampler.remap_topics (include/mvhdp.h mvhdp_remap_topics), built on the host from what the device calls already
return: a similarity from topic_gram, token counts from get_counts, the inactive set from get_alpha.  Pure numpy, K-sized.

A map is an int32 array [K]: map[k] = the topic that takes topic k's tokens, -1 = they become unassigned.  It is applied in one hop and
never chased; compose() makes one map of two.  Not here: the reference's own discriminative-weight delete rule (PTM:773-809) and
splitting a topic."""
import numpy as np

DROP = -1                                                   # MVHDP_UNASSIGNED_TOPIC


def identity_map(K):
    return np.arange(K, dtype=np.int32)


def merge_map(sim, threshold, weight):
    """The connected components of the pairs with sim[i][j] > threshold (strictly; either triangle counts, the diagonal does not), each
    mapped onto its member of the largest weight, equal weights to the lowest id.  A topic in no such pair maps to itself."""
    sim = np.asarray(sim, dtype=np.float64)
    weight = np.asarray(weight)
    K = len(weight)
    if sim.shape != (K, K):
        raise ValueError(f"merge_map: sim must be [{K}][{K}], got {sim.shape}")
    root = list(range(K))

    def find(i):
        while root[i] != i:
            root[i] = root[root[i]]
            i = root[i]
        return i

    for i, j in zip(*np.nonzero(sim > threshold)):
        if i != j:
            a, b = find(int(i)), find(int(j))
            root[max(a, b)] = min(a, b)
    best = {}
    for k in range(K):                                      # ascending k: the first of equal weights is the lowest id
        r = find(k)
        if r not in best or weight[k] > weight[best[r]]:
            best[r] = k
    return np.array([best[find(k)] for k in range(K)], dtype=np.int32)


def prune_map(weight, min_tokens):
    """Topics with weight < min_tokens map to -1 (their tokens become unassigned), the others to themselves."""
    weight = np.asarray(weight)
    out = identity_map(len(weight))
    out[weight < min_tokens] = DROP
    return out


def order_map(weight, inactive=None):
    """A permutation: the active topics by weight descending, equal weights by id, then the inactive topics in id order.  map[k] = the
    new index of topic k."""
    weight = np.asarray(weight)
    K = len(weight)
    off = np.zeros(K, dtype=bool) if inactive is None else np.asarray(inactive).astype(bool)
    order = sorted(range(K), key=lambda k: (bool(off[k]), 0 if off[k] else -weight[k], k))
    out = np.empty(K, dtype=np.int32)
    out[order] = np.arange(K, dtype=np.int32)
    return out


def compose(first, then):
    """One map that does what `first` and then `then` do in two calls: then[first[k]], -1 staying -1."""
    first = np.asarray(first, dtype=np.int32)
    then = np.asarray(then, dtype=np.int32)
    if first.shape != then.shape:
        raise ValueError("compose: the maps differ in length")
    return np.where(first < 0, DROP, then[np.maximum(first, 0)]).astype(np.int32)
