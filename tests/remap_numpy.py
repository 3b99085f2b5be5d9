"""mvhdp_remap_topics restated literally (include/mvhdp.h): (z, alpha, inactive, map, flags) -> (z', alpha', inactive', moved, dropped,
vacated, retired), token by token and topic by topic in plain loops.  Counts are np.bincount of z' and nothing else.  Test
infrastructure: slow on purpose, no vectorised shortcut that could share a mistake with the device code."""
from types import SimpleNamespace

import numpy as np

RETIRE = 0x1


def counts_of(K, V, tokens, z):
    """(n_wk [V][K], n_k [K]) of one view: the recount of z, unassigned tokens left out"""
    on = z >= 0
    nwk = np.bincount(tokens[on].astype(np.int64) * K + z[on], minlength=V * K).reshape(V, K).astype(np.int32)
    return nwk, np.bincount(z[on], minlength=K).astype(np.int32)


def remap(K, z, alpha, inactive, topic_map, flags=0):
    """z: a list of int32 arrays, one per view; alpha [M][K + 1]; inactive [K] uint8.  Returns a namespace of the same, primed."""
    M = len(z)
    topic_map = [int(t) for t in topic_map]
    assert len(topic_map) == K and all(-1 <= t < K for t in topic_map)
    z2, moved, dropped = [], [], []
    for m in range(M):
        out = z[m].copy()
        mv = dr = 0
        for i, old in enumerate(z[m].tolist()):
            if old < 0:
                continue                                     # -1 stays -1
            new = topic_map[old]                             # one hop
            out[i] = new
            mv += new >= 0 and new != old
            dr += new < 0
        z2.append(out); moved.append(mv); dropped.append(dr)
    held = np.zeros(K, dtype=np.int64)                       # tokens per topic before, over all views
    for m in range(M):
        held += np.bincount(z[m][z[m] >= 0], minlength=K)
    alpha2 = np.array(alpha, dtype=np.float64, copy=True)
    inactive2 = np.zeros(K, dtype=np.uint8)
    vacated = retired = 0
    sources_of = [[] for _ in range(K)]                      # {k : map[k] == t}, in ascending k
    for k in range(K):
        if topic_map[k] >= 0:
            sources_of[topic_map[k]].append(k)
    for t in range(K):
        sources = sources_of[t]
        for m in range(M):
            if not sources:
                alpha2[m, t] = 0.0
            else:
                a = alpha[m, sources[0]]                     # a single source moves its bits
                for k in sources[1:]:
                    a = a + alpha[m, k]
                alpha2[m, t] = a
        if sources:
            inactive2[t] = all(inactive[k] for k in sources)
        else:
            inactive2[t] = 1 if (flags & RETIRE) else inactive[t]
            if held[t] > 0 or not inactive[t]:
                vacated += 1
                retired += int(inactive2[t])
    return SimpleNamespace(z=z2, alpha=alpha2, inactive=inactive2, moved=np.array(moved, dtype=np.int64), dropped=np.array(dropped, dtype=np.int64),
                           vacated=vacated, retired=retired)
