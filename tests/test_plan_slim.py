"""Where the planner lets a sweep gather from the 12-bit image of n_wk (SweepPlan::cls[c].narrow == 2; mvhdp_plan.h), without a GPU.
mvhdp_plan_probe speaks for a handle that keeps the image when its tuning says narrow = 2 (as -1 otherwise); whether a handle keeps
it at all -- the lines of a row, the 2^28 bound on a view's types -- is mvhdp_slim_pays, checked in tests/test_slim_layout.py."""
import ctypes as C

from mvtopicmodel_amd import _lib
from tests.helpers import PLAN_REGS

SWEEP_REUSE_TREES, SWEEP_NO_APPLY, SWEEP_FROZEN, SWEEP_LIVE, SWEEP_SEGMENT_APPLY, SWEEP_SEGMENT_OVERLAP = 0x1, 0x2, 0x10, 0x20, 0x40, 0x80
C4 = dict(tok=[80_000_000, 66_000_000, 1_000_000], ent=[550_000, 449_000, 1_000, 0, 0, 0, 0, 0])
C5 = dict(K=1000, M=5, tok=[30_000_000, 40_000_000, 20_000_000, 20_000_000, 0, 0, 0, 5_000_000, 0, 0, 0, 0, 0, 0, 0, 2_000_000],
          ent=[400_000, 400_000, 150_000, 50_000, 3_000, 0, 0, 0], longer=(1_000_000, 900_000, 300_000, 60_000, 4_000), mdt=5000)


def probe(K=400, M=3, D=1_000_000, mdt=250, longer=(1_000_000, 900_000, 40, 0, 0), tok=None, ent=None, flags=0, narrow=2, debug=0,
          trees_current=0, vectors_mix=0, **tuning):
    L = _lib.load_library()
    pi = _lib.PlanInputC()
    pi.num_topics, pi.num_modalities, pi.num_entities, pi.max_entity_tokens = K, M, D, mdt
    for i, v in enumerate(longer):
        pi.entities_longer_than[i] = v
    for i, v in enumerate(tok or []):
        pi.tokens_by_list_rounds[i] = v
    for i, v in enumerate(ent or []):
        pi.entities_by_class[i] = v
    pi.flags, pi.debug, pi.trees_current, pi.num_cus, pi.vectors_mix = flags, debug, trees_current, 256, vectors_mix
    for c in range(6):
        for f in range(3):
            pi.kernel_registers[c][f] = PLAN_REGS[c][f]
    t = _lib.TuningC()
    t.narrow, t.live16, t.live_rows, t.live_overlap = narrow, -1, -1, -1
    for g in range(4):
        t.learnt_walk_step[g] = -1
    for k, v in tuning.items():
        setattr(t, k, v)
    po = _lib.PlanOutputC()
    assert L.mvhdp_plan_probe(C.byref(pi), C.byref(t), C.byref(po)) == 0 and po.status == 0
    return po


def levels(po):
    return [po.class_narrow[c] if po.class_used[c] else None for c in range(6)]


def test_deferred_sweeps_of_long_rows_take_the_image_in_the_one_two_and_four_round_variants():
    po = probe(**C4)                                                         # K = 400: 5 lines against 7
    assert levels(po) == [2, 2, 2, None, None, None]
    assert list(po.class_walk)[:3] == [1, 1, 1]                              # (it belongs to the walk flavour, like the mirror)
    po = probe(**C5)                                                         # K = 1000: 12 lines against 16
    assert [po.class_used[c] for c in range(5)] == [1, 1, 1, 1, 1]
    # the 8- and 16-round variants sit at their register limit and have no such flavour: they stay on the mirror
    assert levels(po)[:5] == [2, 2, 2, 1, 1]
    # segments with the updater catching up in between re-class every row at each rebuild; so does a shard's NO_APPLY sweep
    assert levels(probe(flags=SWEEP_SEGMENT_APPLY, **C4))[:3] == [2, 2, 2]
    assert levels(probe(flags=SWEEP_NO_APPLY, **C4))[:3] == [2, 2, 2]
    assert levels(probe(flags=SWEEP_FROZEN, trees_current=1, **C4))[:3] == [2, 2, 2]
    # trees (and with them mirror and image) that are not this sweep's start counts: neither table
    assert levels(probe(flags=SWEEP_REUSE_TREES, trees_current=0, walk_fixed=1, **C4))[:3] == [0, 0, 0]
    assert levels(probe(flags=SWEEP_REUSE_TREES, trees_current=1, **C4))[:3] == [2, 2, 2]


def test_short_rows_stay_where_they_were():
    for K in (100, 200):                                                     # 2 lines against 2; 3 against 4, but bound by latency (C3)
        kw = dict(K=K, tok=[80_000_000, 66_000_000], ent=[550_000, 450_000])
        with_table, without = probe(**kw), probe(narrow=-1, **kw)
        assert 2 not in levels(with_table)
        assert levels(with_table) == levels(without)


def test_a_handle_without_the_image_and_the_tuning_that_pins_the_tables():
    assert levels(probe(narrow=-1, **C4))[:3] == [1, 1, 1]                   # (a view of 2^28 types or more, or the switch off: no table)
    assert levels(probe(narrow=0, **C4))[:3] == [0, 0, 0]
    assert levels(probe(narrow=1, **C4))[:3] == [1, 0, 0]                    # the mirror for the 1-round variant only


def test_live_overlapped_mix_and_debug_sweeps_never_take_the_image():
    for kw in (dict(flags=SWEEP_LIVE), dict(flags=SWEEP_LIVE, live_rows=0), dict(flags=SWEEP_LIVE, live_rows=0, live16=0),
               dict(flags=SWEEP_LIVE | SWEEP_NO_APPLY), dict(flags=SWEEP_SEGMENT_APPLY | SWEEP_SEGMENT_OVERLAP),
               dict(vectors_mix=1), dict(vectors_mix=1, flags=SWEEP_SEGMENT_APPLY), dict(debug=1)):
        for corpus in (C4, C5):
            po = probe(**kw, **corpus)
            assert 2 not in levels(po), kw
    # (a frozen sweep samples without the mix: the plain flavours, hence the image)
    assert levels(probe(vectors_mix=1, flags=SWEEP_FROZEN, trees_current=1, **C4))[:3] == [2, 2, 2]
