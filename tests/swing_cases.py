"""A forced full swing: the recipe that drives every narrow form of the word-topic counts to the exact limit its comment derives, as
data (no device).  tests/test_swing_cases.py holds it to the oracle and to the planner's own word; tests/test_gpu_count_limits.py runs
every sweep mode over it.

Every entity holds ONE token, in one view; no topic is inactive; alpha[m][k] is 0.0 for every topic but one target t_m.  Removing an
entity's only token empties its topic list (document mass 0), there is no new-topic mass, and the word's tree has one non-zero leaf:
the conditional of WRK:496-535 puts every token of view m into t_m, whatever the random numbers and whatever order the entities are
visited in.  A new target (set_hyper) between two sweeps swings every row whole; the same target again moves nothing.

View 0 (K = 257, odd: the last cell of a row shares a word of the packed forms with the first cell of the next row, or has no partner):

  type  tokens  start                        class       what it reaches
  0     32767   topic 6                      light       a 16-bit delta of -32767 / +32767 in the two halves of one word (6 -> 7)
  1     32767   topic 8                      light       the same in cells of different words (8 -> 7)
  2     32767   topic 256                    light       the unpaired last cell of the row
  3     32768   topic 6                      BIG         the first row beyond the 16-bit delta cells
  4     65534   topic 6                      BIG         the largest cell the 16-bit mirror holds
  5     65535   topic 6                      HEAVY       the first row the mirror gives up
  6     32767   spread over topics 16..31    light       in the 12-bit image before the swing (cells of 2048 and 2047), out of it after
  7     8191    4095 in topic 40, 4096 in 41 light       one cell either side of the 12-bit image's limit, both moving
  8     4096    4095 in topic 50, 1 in 51    light       slim with its largest cell exactly 4095; one token more in a cell after the swing

View 1: type 0 with 32767 tokens in topic 7, type 1 with 100 tokens in topic 3; its targets run the other way round (7 -> 6 while view
0 goes 6 -> 7).

Entity order is type-major, the types in ORDER0: contiguous shards balanced by tokens (tests/helpers.py::shards_of) then hold most
types whole and cut a light row of 32767 tokens in two, so that partial deltas of several members add up to +-32767."""
import numpy as np

from mvtopicmodel_amd.native import Hyper
from mvtopicmodel_amd.synth import Corpus

K = 257
V = [9, 2]
# view 0: {type: {topic: tokens}}
START0 = {
    0: {6: 32767},
    1: {8: 32767},
    2: {256: 32767},
    3: {6: 32768},
    4: {6: 65534},
    5: {6: 65535},
    6: {k: 2048 - (k == 31) for k in range(16, 32)},
    7: {40: 4095, 41: 4096},
    8: {50: 4095, 51: 1},
}
START1 = {0: {7: 32767}, 1: {3: 100}}
ORDER0 = [4, 5, 3, 0, 6, 1, 7, 2, 8]             # 2 shards cut type 0, 3 shards cut types 5 (heavy) and 1 (light)
LIMIT_ROWS = {0: 32767, 1: 32767, 2: 32767, 3: 32768, 4: 65534, 5: 65535, 6: 32767}     # view 0: the totals nothing may move by one
TOKENS_OF_THE_LIMIT_ROWS_AND_VIEW_1 = 327_772
# (view 0, view 1) targets of the sweeps; step 1 repeats step 0's: an idle sweep (a group of shards agrees on its packed exchange behind
# it, so steps 2 to 5 travel packed: the last cell, and both sign orders in the two halves of one word)
TARGETS = [(7, 6), (7, 6), (256, 7), (6, 256), (7, 6), (6, 7)]
IDLE_STEPS = (1,)
FOLLOW_UP = (9, 8)                                # one more deferred sweep behind a mode that keeps the mirror current by deltas or atomics
ROW_BIG, ROW_HEAVY, ROW_SLIM = 2, 1, 4            # MVHDP_ROW_* of mvhdp_device.h (the weight class in bits 0-1, the 12-bit image in bit 2)
TUNING = dict(walk_fixed=1, walk_theta=[0.3, 0.3])   # the deferred modes of tests/test_gpu_count_limits.py sweep with this


def tokens_of(m):
    return {w: sum(cells.values()) for w, cells in (START0, START1)[m].items()}


def _view(start, order):
    types = np.concatenate([np.full(sum(start[w].values()), w, dtype=np.int32) for w in order])
    z = np.concatenate([np.full(n, k, dtype=np.int32) for w in order for k, n in sorted(start[w].items())])
    return types, z


def corpus():
    """(the corpus, the start assignments): view 0's entities first, one token each, then view 1's"""
    t0, z0 = _view(START0, ORDER0)
    t1, z1 = _view(START1, [0, 1])
    n0, n1 = len(t0), len(t1)
    off0 = np.concatenate([np.arange(n0 + 1), np.full(n1, n0)]).astype(np.int64)
    off1 = np.concatenate([np.zeros(n0, dtype=np.int64), np.arange(n1 + 1)]).astype(np.int64)
    return Corpus(K, list(V), [off0, off1], [t0, t1], "swing"), [z0, z1]


def hyper_for(targets):
    """alpha 0.0 everywhere but at the view's target"""
    hy = Hyper.defaults(K, V)
    hy.alpha[:, :K] = 0.0
    for m, t in enumerate(targets):
        hy.alpha[m, t] = 0.1
    return hy


def counts_of(c, z):
    """[(n_wk, n_k)] per view of the assignments z (tokens with z = -1 counted nowhere)"""
    out = []
    for m in range(c.M):
        on = z[m] >= 0
        nwk = np.bincount(c.tokens[m][on].astype(np.int64) * K + z[m][on], minlength=V[m] * K).reshape(V[m], K).astype(np.int32)
        out.append((nwk, nwk.sum(axis=0).astype(np.int32)))
    return out


def expected_for(targets, c):
    """the closed form: (z per view, [(n_wk, n_k)] per view) after a sweep towards `targets` -- every z is its view's target"""
    z = [np.full(len(c.tokens[m]), targets[m], dtype=np.int32) for m in range(c.M)]
    return z, counts_of(c, z)


def expected_after(step, c):
    return expected_for(TARGETS[step], c)


def guard_start(c, z0):
    """the same start with a tenth of type 0's tokens of view 0 unassigned (every tenth of them)"""
    z = [a.copy() for a in z0]
    idx = np.flatnonzero(c.tokens[0] == 0)[::10]
    z[0][idx] = -1
    return z


def row_classes(nwk_all):
    """MvModel::heavy as a tree build writes it from the counts [rows of all views][K]"""
    tot, big = nwk_all.sum(axis=1), nwk_all.max(axis=1)
    return np.where(tot > 65534, ROW_HEAVY, np.where(tot > 32767, ROW_BIG, 0)) | np.where(big <= 4095, ROW_SLIM, 0)


def plan_input(c, known, flags=0, unassigned=False):
    """mvhdp_plan_input of the recipe, as tests/census_cases.py::plan_input builds one: topic lists of one topic each, their sizes
    unknown (the first sweep after build_counts) or known"""
    from mvtopicmodel_amd import _lib
    from tests.helpers import PLAN_REGS
    tot = sum(np.diff(np.asarray(o)) for o in c.doc_off)
    pi = _lib.PlanInputC()
    pi.num_topics, pi.num_modalities, pi.num_entities, pi.max_entity_tokens = c.K, c.M, c.D, int(tot.max())
    for q in range(5):
        pi.entities_longer_than[q] = int((tot > (64 << q)).sum())
    if known:
        pi.entities_by_class[0] = c.D
        pi.tokens_by_list_rounds[0] = int(tot.sum())
    pi.flags, pi.num_cus, pi.unassigned = flags, 256, int(unassigned)
    for q in range(6):
        for f in range(3):
            pi.kernel_registers[q][f] = PLAN_REGS[q][f]
    return pi
