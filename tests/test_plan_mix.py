"""The planner with a useVectorsLambda mix set (mvhdp_plan_input.vectors_mix), without a GPU: the mix flavours are the walk flavour
of every class, sized from their own register counts; a live sweep takes its stored-tree form; and with vectors_mix = 0 every plan is
what it is without the field (the two calls are compared with each other, not against constants)."""
import ctypes as C

import pytest

from mvtopicmodel_amd import _lib
from tests.test_plan import REGS, SWEEP_FROZEN, SWEEP_LIVE, SWEEP_NO_APPLY, SWEEP_REUSE_TREES, SWEEP_SEGMENT_APPLY

OUT_FIELDS = [f for f, _ in _lib.PlanOutputC._fields_]


def probe(vectors_mix=None, regs_mix=None, K=400, M=3, D=1_000_000, mdt=250, longer=(1_000_000, 900_000, 40, 0, 0), tok=None, ent=None, flags=0,
          tuning=None, batch=0, debug=0, trees_current=0, inactive=0):
    L = _lib.load_library()
    pi = _lib.PlanInputC()
    pi.num_topics, pi.num_modalities, pi.num_entities, pi.max_entity_tokens = K, M, D, mdt
    for i, v in enumerate(longer):
        pi.entities_longer_than[i] = v
    for i, v in enumerate(tok or []):
        pi.tokens_by_list_rounds[i] = v
    for i, v in enumerate(ent or []):
        pi.entities_by_class[i] = v
    pi.flags, pi.debug, pi.batch, pi.trees_current, pi.num_cus = flags, debug, batch, trees_current, 256
    pi.inactive_topics = inactive
    for c in range(6):
        for f in range(3):
            pi.kernel_registers[c][f] = REGS[c][f]
    if vectors_mix is not None:                       # (None: the field is left as the zero-initialised structure has it)
        pi.vectors_mix = vectors_mix
    for c, row in enumerate(regs_mix or []):
        for f in range(3):
            pi.kernel_registers_mix[c][f] = row[f]
    t = None
    if tuning:
        t = _lib.TuningC()
        t.narrow = t.live16 = t.live_rows = t.live_overlap = -1
        for g in range(4):
            t.learnt_walk_step[g] = -1
        for k, v in tuning.items():
            if isinstance(v, (list, tuple)):
                for i, x in enumerate(v):
                    getattr(t, k)[i] = x
            else:
                setattr(t, k, v)
    po = _lib.PlanOutputC()
    assert L.mvhdp_plan_probe(C.byref(pi), C.byref(t) if t is not None else None, C.byref(po)) == 0
    return po


def as_tuple(po):
    out = []
    for f in OUT_FIELDS:
        v = getattr(po, f)
        out.append(tuple(v) if hasattr(v, "__len__") else v)
    return tuple(out)


# the inputs tests/test_plan.py records
C4_EARLY = dict(tok=[6_000_000, 140_000_000, 1_000_000, 200_000], ent=[40_000, 950_000, 10_000, 0, 0, 0, 0, 0])
C4_SETTLED = dict(tok=[80_000_000, 66_000_000, 1_000_000], ent=[550_000, 449_000, 1_000, 0, 0, 0, 0, 0])
C5 = dict(K=1000, M=5, tok=[30_000_000, 40_000_000, 20_000_000, 20_000_000], ent=[400_000, 400_000, 150_000, 50_000, 0, 0, 0, 0],
          tuning=dict(tree_branch_share=[0.44, 0.45, 0.45, 0.45, 0.45]))
RECORDED = [
    C4_EARLY, C4_SETTLED, C5,
    dict(tuning=dict(walk_fixed=1, walk_theta=[0.5, 0.0, 0.0]), **C4_SETTLED),
    dict(flags=SWEEP_LIVE, tok=[80_000_000, 66_000_000], ent=[550_000, 450_000]),
    dict(flags=SWEEP_LIVE, tok=[80_000_000, 66_000_000], ent=[550_000, 450_000], tuning=dict(live_rows=0)),
    dict(flags=SWEEP_LIVE, inactive=1, tok=[80_000_000, 66_000_000], ent=[550_000, 450_000]),
    dict(flags=SWEEP_SEGMENT_APPLY, **C4_SETTLED), dict(flags=SWEEP_NO_APPLY, **C4_SETTLED), dict(flags=SWEEP_FROZEN | SWEEP_REUSE_TREES, trees_current=1, **C4_SETTLED),
    dict(batch=1, tok=[146_000_000, 1_000_000], ent=[990_000, 10_000, 0, 0, 0, 0, 0, 0]),
    dict(K=200, tok=[80_000_000, 66_000_000], ent=[550_000, 450_000], tuning=dict(learnt_walk_step=[-1, -1, 0, -1], tree_branch_share=[0.2, 0.6, 0.6])),
    dict(debug=1, **C4_EARLY), dict(tuning=dict(force_primary=32), **C4_EARLY), dict(tuning=dict(force_primary=4), **C4_EARLY),
    dict(K=2048, M=8, mdt=5000, longer=(10, 10, 10, 10, 5), D=10),
]


@pytest.mark.parametrize("i", range(len(RECORDED)))
def test_mix_off_is_todays_plan(i):
    kw = RECORDED[i]
    a, b = probe(vectors_mix=None, **kw), probe(vectors_mix=0, regs_mix=[(250, 250, 250)] * 6, **kw)
    assert as_tuple(a) == as_tuple(b)                  # (the mix flavours' registers are not looked at either)


def test_live_with_a_mix_is_the_stored_tree_form():
    kw = dict(flags=SWEEP_LIVE, tok=[80_000_000, 66_000_000], ent=[550_000, 450_000])
    off, on = probe(**kw), probe(vectors_mix=1, **kw)
    stored = probe(tuning=dict(live_rows=0), **kw)
    assert off.live_rows == 1 and off.segments == 1
    assert on.status == 0 and on.live_rows == 0 and on.segments == stored.segments == 4
    assert as_tuple(on) == as_tuple(probe(vectors_mix=1, tuning=dict(live_rows=1), **kw))       # whatever the tuning says
    # the 16-bit mirror form works with a mix as it does without
    assert [on.class_narrow[c] for c in range(2)] == [stored.class_narrow[c] for c in range(2)] == [1, 1]
    # a FROZEN sweep does not sample with the mix: today's plan
    kf = dict(flags=SWEEP_FROZEN | SWEEP_REUSE_TREES, trees_current=1, **C4_SETTLED)
    assert as_tuple(probe(vectors_mix=1, **kf)) == as_tuple(probe(**kf))


@pytest.mark.parametrize("kw", [C4_EARLY, C4_SETTLED, C5, dict(flags=SWEEP_SEGMENT_APPLY, **C4_SETTLED), dict(flags=SWEEP_NO_APPLY, **C4_SETTLED)])
def test_deferred_plans_name_the_same_classes(kw):
    off, on = probe(**kw), probe(vectors_mix=1, **kw)
    assert on.status == 0
    for f in ("segments", "primary_class", "register_resident", "dominant_class", "routed_prefix", "delta16", "live_rows"):
        assert getattr(on, f) == getattr(off, f), f
    for f in ("class_used", "class_map", "class_stream", "class_register_resident", "class_lds_bytes"):
        assert tuple(getattr(on, f)) == tuple(getattr(off, f)), f
    # the mix is compiled for the walk flavour only: every register-resident class runs it
    assert all(on.class_walk[c] == 1 for c in range(5) if on.class_used[c] and on.class_register_resident[c])


def test_grids_follow_the_mix_flavours_registers():
    regs_mix = [(0, 80, 96), (0, 80, 104), (0, 128, 160), (0, 226, 256), (0, 256, 256), (96, 96, 128)]
    off = probe(**C4_SETTLED)
    same = probe(vectors_mix=1, **C4_SETTLED)          # no counts named: sized as the plain flavours
    on = probe(vectors_mix=1, regs_mix=regs_mix, **C4_SETTLED)
    assert off.class_grid[0] == same.class_grid[0] == 256 * 7       # 72 VGPRs: 7 waves per SIMD
    assert on.class_grid[0] == 256 * 6                              # 80: 6
    assert on.class_grid[1] == 256 * 6
