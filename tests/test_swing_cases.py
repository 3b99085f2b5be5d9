"""tests/swing_cases.py held to the oracle and to the planner's own word, without a device: the recipe really swings every limit row
whole at every step -- cell deltas of exactly -+32767, -+32768, -+65534 and -+65535 --, its closed form is the oracle's state, and the
plain deferred sweep of tests/test_gpu_count_limits.py is planned on the 16-bit delta cells unless a token may be unassigned.  So the
device test cannot pass vacuously after an edit of the recipe: a limit row one token off fails here."""
import ctypes as C

import numpy as np
import pytest

from mvtopicmodel_amd.native import SWEEP_LIVE, SWEEP_LIVE_SEGMENTS, SWEEP_NO_APPLY, SWEEP_SEGMENT_APPLY
from tests import census_cases as cc
from tests import swing_cases as sw
from tests.helpers import make_oracle, shards_of


@pytest.fixture(scope="module")
def chain():
    """the oracle's deferred chain over TARGETS: per step its statistics, the n_wk of view 0 before and after, and z after"""
    c, z0 = sw.corpus()
    o = make_oracle(c, sw.hyper_for(sw.TARGETS[0]))
    for m in range(c.M):
        o.set_assignments(m, z0[m])
    o.build_counts()
    steps = []
    for it, t in enumerate(sw.TARGETS):
        hy = sw.hyper_for(t)
        o.set_hyper(hy.alpha, hy.alpha_sum, hy.beta, hy.beta_sum, hy.gamma, hy.p_a, hy.p_b, hy.inactive)
        before = o.get_counts(0)[0].copy()
        st = o.sweep(it, 77)["stats"]
        steps.append(dict(stats=st, before=before, z=[o.get_assignments(m) for m in range(c.M)], counts=[o.get_counts(m) for m in range(c.M)]))
    o.close()
    return c, z0, steps


def test_the_recipe_is_the_table_of_its_docstring():
    c, z0 = sw.corpus()
    n0 = sw.tokens_of(0)
    assert {w: n0[w] for w in sw.LIMIT_ROWS} == sw.LIMIT_ROWS == {0: 32767, 1: 32767, 2: 32767, 3: 32768, 4: 65534, 5: 65535, 6: 32767}
    assert sum(sw.LIMIT_ROWS.values()) + sum(sw.tokens_of(1).values()) == sw.TOKENS_OF_THE_LIMIT_ROWS_AND_VIEW_1
    assert c.K == 257 and c.K % 2 == 1 and c.D == c.total_tokens
    assert all((np.diff(c.doc_off[0]) + np.diff(c.doc_off[1]) == 1))                     # one token an entity, in one view
    nwk0 = sw.counts_of(c, z0)[0][0]
    assert np.array_equal(np.bincount(c.tokens[0], minlength=sw.V[0]), [n0[w] for w in range(sw.V[0])])
    assert np.array_equal(sw.row_classes(nwk0) & 3, [0, 0, 0, sw.ROW_BIG, sw.ROW_BIG, sw.ROW_HEAVY, 0, 0, 0])
    assert sorted(nwk0[6][nwk0[6] > 0]) == [2047] + [2048] * 15 and nwk0[6][16:32].all()
    assert (nwk0[7][40], nwk0[7][41], nwk0[7].sum()) == (4095, 4096, 8191)
    assert (nwk0[8].max(), nwk0[8].sum()) == (4095, 4096)
    assert np.array_equal((sw.row_classes(nwk0) & sw.ROW_SLIM) != 0, [0, 0, 0, 0, 0, 0, 1, 0, 1])
    # both halves of one word in both sign orders (6 <-> 7; view 1 the other way), cells of different words (8 -> 7), the unpaired last cell
    assert sw.TARGETS[0] == (7, 6) and sw.TARGETS[1] == sw.TARGETS[0] and sw.TARGETS[2][0] == c.K - 1 and sw.TARGETS[3][1] == c.K - 1
    assert sw.TARGETS[3][0] == 6 and sw.TARGETS[4] == (7, 6) and sw.TARGETS[5] == (6, 7)
    assert 6 // 2 == 7 // 2 and 8 // 2 != 7 // 2
    # a row whose last cell shares a word of the packed mirror with the next row's first cell: the even rows of an odd K -- types 0 and
    # 2, both of 32767 tokens that pass through topic 256
    for row in (0, 2):
        assert (row * c.K + c.K - 1) // 2 == ((row + 1) * c.K) // 2


def test_contiguous_shards_cut_a_light_limit_row():
    """partial deltas of several members must add up to +-32767 in a row that travels packed"""
    c, z0 = sw.corpus()
    for n in (2, 3):
        parts = [np.bincount(sub.tokens[0], minlength=sw.V[0]) for _, sub, _ in shards_of(c, z0, n)]
        cut = [w for w in range(sw.V[0]) if sum(p[w] > 0 for p in parts) > 1]
        assert any(sw.tokens_of(0)[w] == 32767 for w in cut), (n, cut)
        assert all(sum(p) > 0 for p in parts)


def test_the_oracle_swings_every_limit_row_whole(chain):
    c, z0, steps = chain
    n0 = sw.tokens_of(0)
    for it, s in enumerate(steps):
        st = s["stats"]
        assert st["tokens"] == c.total_tokens
        assert st["changed"] == (0 if it in sw.IDLE_STEPS else c.total_tokens), it       # every token is movable, and moves
        assert st["new_mass_cnt"] == 0 and st["topic_doc_mass_cnt"] == 0
        d = s["counts"][0][0].astype(np.int64) - s["before"]
        for w, n in sw.LIMIT_ROWS.items():
            if it in sw.IDLE_STEPS:
                assert not d[w].any()
            elif w == 6 and it == 0:
                assert (d[w].min(), d[w].max()) == (-2048, 32767)
            else:
                assert (d[w].min(), d[w].max()) == (-n, n), (it, w)
        assert (d[7].min(), d[7].max()) == ((-4096, 8191) if it == 0 else (0, 0) if it in sw.IDLE_STEPS else (-8191, 8191))
        # the closed form
        z, counts = sw.expected_after(it, c)
        for m in range(c.M):
            assert np.array_equal(s["z"][m], z[m]), (it, m)
            assert np.array_equal(s["counts"][m][0], counts[m][0]) and np.array_equal(s["counts"][m][1], counts[m][1]), (it, m)
    # type 6 is in the 12-bit image before the first swing and not after; type 8 leaves it by one token in a cell
    before, after = sw.row_classes(steps[0]["before"]), sw.row_classes(steps[0]["counts"][0][0])
    assert before[6] & sw.ROW_SLIM and not after[6] & sw.ROW_SLIM
    assert before[8] & sw.ROW_SLIM and steps[0]["before"][8].max() == 4095 and steps[0]["counts"][0][0][8].max() == 4096 and not after[8] & sw.ROW_SLIM
    assert n0[5] == 65535


def probe(pi, tuning):
    from mvtopicmodel_amd import _lib
    po = _lib.PlanOutputC()
    assert _lib.load_library().mvhdp_plan_probe(C.byref(pi), C.byref(cc.probe_tuning(tuning, {})), C.byref(po)) == 0 and po.status == 0
    return po


@pytest.mark.parametrize("force", [0, 1, 2])
def test_the_planner_puts_the_plain_deferred_sweep_on_the_16_bit_delta_cells(force):
    c, _ = sw.corpus()
    tuning = dict(force_primary=force, **sw.TUNING)
    for known in (False, True):
        po = probe(sw.plan_input(c, known), tuning)
        assert po.delta16 == 1, (force, known)
        served = po.class_map[0]                                          # every entity's list holds one topic
        assert po.register_resident == 1 and po.class_register_resident[served] == 1 and po.class_narrow[served] != 0
        # once a token may be unassigned a row's total can grow: no 16-bit delta cells
        assert probe(sw.plan_input(c, known, unassigned=True), tuning).delta16 == 0
        # the other modes never use them (the deltas leave the handle, or land segment by segment)
        for flags in (SWEEP_NO_APPLY, SWEEP_SEGMENT_APPLY | SWEEP_LIVE_SEGMENTS(3), SWEEP_LIVE):
            assert probe(sw.plan_input(c, known, flags=flags), tuning).delta16 == 0
        assert probe(sw.plan_input(c, known), dict(narrow=0, **tuning)).delta16 == 0
