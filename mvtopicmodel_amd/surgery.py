"""Topic maps for NativeSampler.remap_topics (include/mvhdp.h mvhdp_remap_topics), built on the host from what the device calls already
return: a similarity from topic_gram, token counts from get_counts, the inactive set from get_alpha.  Pure numpy, K-sized.

A map is an int32 array [K]: map[k] = the topic that takes topic k's tokens, -1 = they become unassigned.  It is applied in one hop and
never chased; compose() makes one map of two.  Not here: the reference's own discriminative-weight delete rule (PTM:773-809).

For NativeSampler.split_topic (mvhdp_split_topic): free_topics() lists the indices a split may take, hint_from_words() builds one view's
hint row."""
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


def free_topics(n_k_total, inactive, alpha):
    """The indices a split may take as its target when it picks one itself, ascending: topics of the inactive set that hold no token in any
    view (n_k_total [K], summed over the views) and whose alpha (alpha [M][K] or [M][K + 1]) is exactly 0.0 in every view.  split_topic
    with target=None takes the first."""
    n = np.asarray(n_k_total)
    K = len(n)
    off = np.asarray(inactive).astype(bool)
    a = np.asarray(alpha, dtype=np.float64)
    a = a.reshape(-1, a.shape[-1])[:, :K]
    if off.shape != (K,) or a.shape[1] != K:
        raise ValueError("free_topics: n_k_total, inactive and alpha disagree about K")
    return np.flatnonzero(off & (n == 0) & (a == 0.0).all(axis=0)).astype(np.int32)


def hint_from_words(V, stay=(), go=()):
    """One view's type_hint row [V] int8 for split_topic: -1 everywhere, 0 for the types in `stay` (they stay in the source), 1 for those
    in `go` (they start in the target).  A type in both lists is an error."""
    stay = np.asarray(list(stay), dtype=np.int64)
    go = np.asarray(list(go), dtype=np.int64)
    for name, x in (("stay", stay), ("go", go)):
        if len(x) and (x.min() < 0 or x.max() >= V):
            raise ValueError(f"hint_from_words: a type of `{name}` is outside [0, {V})")
    if len(np.intersect1d(stay, go)):
        raise ValueError("hint_from_words: a type is in both lists")
    row = np.full(V, -1, dtype=np.int8)
    row[stay] = 0
    row[go] = 1
    return row
