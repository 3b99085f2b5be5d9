"""Inputs of the cohort tests (mvhdp_cohort_top_words), made on the host alone.  Test infrastructure.

The hand-sized corpus of tests/test_cohort_kats.py is HAND_*; the device cases are three-view corpora of a few thousand tokens whose
shapes sit on the borders of the device code: the 64 lanes of a wave, the four-wave split of the selection, a partial last chunk."""
from types import SimpleNamespace

import numpy as np

from mvtopicmodel_amd.native import Hyper

K_VALUES = [1, 5, 63, 64, 65, 400]
V_VALUES = [1, 63, 64, 65, 257, 1000]
SPANS = [0, 1, 64, 65, 700]                     # every case holds an entity of each length in views 0 and 1

# ---- the hand-sized corpus: 6 entities, 2 views, K = 3 -------------------------------------------------------------------------------
HAND_K = 3
HAND_V = [6, 4]
# view 0, per entity a list of (type, z); entity 3 lacks the view; z = -1 is unassigned, type 6 and 9 are out of the vocabulary
HAND_DOCS0 = [
    [(0, 0), (0, 0), (1, 0), (2, 1), (5, 2)],
    [(0, 0), (1, 0), (1, 1), (3, 1), (3, -1), (6, 1)],
    [(2, 1), (2, 1), (4, 0), (5, 2), (5, 2)],
    [],
    [(0, 0), (3, 0), (4, 0), (9, 2), (2, -1)],
    [(1, 1), (4, 1), (4, 0), (0, 2)],
]
HAND_DOCS1 = [[(0, 0)], [], [(1, 1), (1, 1)], [(3, 2)], [], [(2, 0), (0, 0)]]


def hand_view(docs):
    off = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    tok = np.array([t for d in docs for t, _ in d], dtype=np.int32)
    z = np.array([k for d in docs for _, k in d], dtype=np.int32)
    return off, tok, z


# ---- device cases ---------------------------------------------------------------------------------------------------------------------
def make(K, V, seed=0, extra=30, holes=True):
    """A corpus of len(V) views over D = len(SPANS) + extra entities.  Views 0 and 1 hold one entity of every length of SPANS (at
    different entities) and short entities besides; a few entities lack a view.  Types and topics are geometric draws, so a topic's head
    words repeat and the tail ties at small counts.  holes: a few tokens of views 0 and 1 are unassigned (-1) or out of the vocabulary."""
    rng = np.random.default_rng(1000003 * K + 101 * V[0] + seed)
    M, D = len(V), len(SPANS) + extra
    c = SimpleNamespace(K=K, V=list(V), M=M, D=D, doc_off=[], tokens=[], z=[])
    for m in range(M):
        lens = rng.integers(0, 40, D)
        lens[rng.random(D) < 0.1] = 0
        if m < 2:
            lens[rng.permutation(D)[:len(SPANS)]] = SPANS
        else:
            lens = np.minimum(lens, 5)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        N = int(off[-1])
        tok = np.minimum(rng.geometric(min(0.5, 8.0 / V[m]), N) - 1, V[m] - 1).astype(np.int32)
        z = np.minimum(rng.geometric(min(0.5, 6.0 / K), N) - 1, K - 1).astype(np.int32)
        if K >= 3:
            z[z == 1] = K - 1                                                # topic 1 holds nothing: empty lists, all padding
        if holes and m < 2 and N > 20:
            at = rng.permutation(N)[:8]
            z[at[:4]] = -1
            tok[at[4:]] = V[m] + np.arange(4) * 3
        c.doc_off.append(off); c.tokens.append(tok); c.z.append(z)
    c.hy = Hyper.defaults(K, V)
    return c


def cohorts(c, seed=0):
    """none, one entity, one entity three times, two overlapping parts, everything, a random draw with repeats, the longest entities,
    the last and the first entity: an odd number of cohorts, so that passes of two leave one over"""
    rng = np.random.default_rng(seed + c.D)
    D = c.D
    longest = [int(np.argmax(np.diff(c.doc_off[m]))) for m in range(2)]
    return [[], [int(rng.integers(D))], [longest[0]] * 3, list(range(0, 2 * D // 3)), list(range(D // 3, D)), list(range(D)),
            [int(x) for x in rng.integers(0, D, D // 2)], longest + longest[::-1], [D - 1, 0]]


def table_bytes(c, m):
    return 4 * c.K * c.V[m]
