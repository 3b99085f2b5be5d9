"""Recipes for the launch census (NativeSampler.sweep_census): for every compiled sweep kernel the smallest case that makes the planner
(mvhdp_plan.h) and the resolve rule (mvhdp_flavour.h) launch it over tokens, plus one on either side of every K at which they switch
kernels.  tests/test_census_cases.py holds the table to the planner's own word without a device; tests/test_gpu_flavour_census.py runs
every recipe against its reference with the census as witness.

A key is the kernel's template arguments (rmax, debug, walk, narrow, roomy, liverows, mix); rmax 0 is the generic kernel.

How a recipe steers:
  force_primary = R on entities of at most 64 R - 1 tokens, the longest of them with more than 32 R topics in their lists: the R-round
      variant serves every entity, nothing is routed, and its rounds beyond R / 2 hold slots
  PLAIN   thresholds handed back as "searched, 0" (learnt_walk_step) with a tree-branch share that is steered: no threshold, no
          measuring sweep -- the plain flavour from the first sweep on where the mirror does not pay (K < 256, or narrow = 0)
  WALK    a fixed threshold: the walk flavour
  MVHDP_SLIM=0 at create: a handle without the 12-bit image, so that the 1-, 2- and 4-round variants stay on the 16-bit mirror
  live sweeps run as one wavefront (single_wave), which is what the sequential oracle restates; the kernel is the same instantiation."""
from collections import namedtuple

import numpy as np

from mvtopicmodel_amd.native import SWEEP_FROZEN, SWEEP_GENERIC_KERNEL, SWEEP_LIVE, SWEEP_LIVE_SEGMENTS, SWEEP_SEGMENT_APPLY, Hyper
from mvtopicmodel_amd.synth import Corpus

# mode: which reference a sweep is compared with, and how --
#   deferred   Oracle.sweep                       (tests/test_gpu_parity.py)
#   segmented  oracle_segmented_sweep             (tests/test_gpu_segmented.py)
#   frozen     Oracle.sweep with SWEEP_FROZEN     (tests/test_gpu_parity.py::test_sweep_many_equals_single_sweeps)
#   live       Oracle.sweep_live_seq, one wave    (tests/test_gpu_live.py::test_one_wave_live_sweep_equals_the_sequential_oracle)
#   mix        MixRef.sweep                       (tests/test_gpu_vectors_mix.py)
Recipe = namedtuple("Recipe", "name key K R mode flags tuning env dbg")

V = [600, 40]
SEGMENTS = 3
MIX_LAMBDA = 0.25
PLAIN = dict(learnt_walk_step=[0, 0, 0, -1], tree_branch_share=[0.1] * 8)
WALK = dict(walk_fixed=1, walk_theta=[0.3, 0.3])
NO_SLIM = {"MVHDP_SLIM": "0"}
K_OF = {1: 400, 2: 400, 4: 400, 8: 500, 16: 1000}         # 256 <= K (the mirror pays); K <= 512 up to 8 rounds: rows of one batch


def corpus(K, R):
    """Two views, fifteen entities: three of 40 R .. 64 R - 1 tokens -- topic lists beyond half the R-round variant's slots, none beyond
    them -- and a dozen short ones.  (The generic kernel's recipes take R = 1.)"""
    rng = np.random.RandomState(9 + R)
    lens0 = np.array([64 * R - 9, 25, 48 * R, 40 * R] + [25] * 11, dtype=np.int64)
    lens1 = rng.randint(0, 9, len(lens0)).astype(np.int64)
    off = [np.concatenate([[0], np.cumsum(l)]) for l in (lens0, lens1)]
    return Corpus(K, V, off, [rng.randint(0, V[m], off[m][-1]).astype(np.int32) for m in range(2)])


def hyper(K):
    return Hyper.defaults(K, V)


def list_lengths(c, z):
    """topics with a token in any view, per entity: the length of its topic list"""
    return [len(np.unique(np.concatenate([z[m][c.doc_off[m][d]:c.doc_off[m][d + 1]] for m in range(c.M)]))) for d in range(c.D)]


def _r(name, key, K, R, mode="deferred", flags=0, tuning=None, env=None, dbg=False):
    t = dict(force_primary=R)
    t.update(tuning or {})
    return Recipe(name, tuple(key), K, R, mode, flags, t, dict(env or {}), dbg)


def _live(name, key, K, R, live16):
    return _r(name, key, K, R, "live", SWEEP_LIVE | SWEEP_LIVE_SEGMENTS(1), dict(live16=live16, live_rows=1, single_wave=1))


def _recipes():
    out = []
    for R in (1, 2, 4, 8, 16):
        K = K_OF[R]
        two = {1: 600, 2: None, 4: 600, 8: 600, 16: 1024}[R]      # rows of two batches: 512 < K <= 1024 (the 2-round variant: its ROOMY build, below)
        one = 1025 if R == 16 else K                              # sixteen rounds of slots need K > 512: rows of one batch again beyond 1024
        out += [
            _r(f"r{R}-plain", (R, 0, 0, 0, 0, 0, 0), K, R, tuning=dict(narrow=0, **PLAIN)),
            _r(f"r{R}-walk32", (R, 0, 1, 0, 0, 0, 0), K, R, tuning=dict(narrow=0, **WALK)),
            _r(f"r{R}-debug", (R, 1, 1, 0, 0, 0, 0), K, R, dbg=True),
            _r(f"r{R}-mirror", (R, 0, 1, 1, 0, 0, 0), K, R, env=NO_SLIM),
            _live(f"r{R}-live32", (R, 0, 1, 0, 0, 1, 0), K, R, 0),
            _live(f"r{R}-live16", (R, 0, 1, 1, 0, 1, 0), one, R, 1),
            _r(f"r{R}-mix32", (R, 0, 1, 0, 0, 0, 1), K, R, "mix", tuning=dict(narrow=0)),
            _r(f"r{R}-mix-debug", (R, 1, 1, 0, 0, 0, 1), K, R, "mix", dbg=True),
            _r(f"r{R}-mix-mirror", (R, 0, 1, 1, 0, 0, 1), K, R, "mix"),
        ]
        if two:
            out.append(_live(f"r{R}-live16-two-batches", (R, 0, 1, 1, 0, 2, 0), two, R, 1))
        if R <= 4:
            out.append(_r(f"r{R}-slim", (R, 0, 1, 2, 0, 0, 0), K, R))
    # the 2-round variant's builds for six waves a SIMD (K >= 512 on the mirror)
    out += [
        _r("r2-roomy-mirror", (2, 0, 1, 1, 1, 0, 0), 600, 2, env=NO_SLIM),
        _r("r2-roomy-slim", (2, 0, 1, 2, 1, 0, 0), 600, 2),
        _live("r2-roomy-live16", (2, 0, 1, 1, 1, 2, 0), 600, 2, 1),
    ]
    # the generic kernel's four builds
    for dbg in (0, 1):
        out.append(_r("generic" + "-debug" * dbg, (0, dbg, 0, 0, 0, 0, 0), 100, 1, flags=SWEEP_GENERIC_KERNEL, tuning=dict(force_primary=0), dbg=bool(dbg)))
        out.append(_r("generic-mix" + "-debug" * dbg, (0, dbg, 0, 0, 0, 0, 1), 100, 1, "mix", SWEEP_GENERIC_KERNEL, dict(force_primary=0), dbg=bool(dbg)))
    # ---- either side of every K at which the rule or the planner switches kernels ----
    # 255 | 256: the mirror starts to pay without a threshold
    out += [_r("k255-plain", (1, 0, 0, 0, 0, 0, 0), 255, 1, tuning=PLAIN), _r("k256-mirror", (1, 0, 1, 1, 0, 0, 0), 256, 1, tuning=PLAIN)]
    # 511 | 512 | 513 in the 2-round variant: ROOMY, on the mirror, on the 12-bit image, and with live rows (K = 512: the two-batch build
    # over rows of one batch)
    for K in (511, 512, 513):
        ro = int(K >= 512)
        out += [_r(f"k{K}-r2-mirror", (2, 0, 1, 1, ro, 0, 0), K, 2, env=NO_SLIM),
                _r(f"k{K}-r2-slim", (2, 0, 1, 2, ro, 0, 0), K, 2),
                _live(f"k{K}-r2-live16", (2, 0, 1, 1, ro, 2 if ro else 1, 0), K, 2, 1)]
    # 1024 | 1025 with live rows: two batches back to three or more (the base recipes of sixteen rounds sit on these; eight rounds too)
    out += [_live("k1024-r8-live16", (8, 0, 1, 1, 0, 2, 0), 1024, 8, 1), _live("k1025-r8-live16", (8, 0, 1, 1, 0, 1, 0), 1025, 8, 1)]
    # a multiple of 85 for the 12-bit image: 340 cells fill four lines, 341 take a fifth
    out += [_r(f"k{K}-r4-slim", (4, 0, 1, 2, 0, 0, 0), K, 4) for K in (340, 341)]
    # ---- the other deferred modes, on kernels named above ----
    out += [
        _r("r2-mirror-segmented", (2, 0, 1, 1, 0, 0, 0), 400, 2, "segmented", SWEEP_SEGMENT_APPLY | SWEEP_LIVE_SEGMENTS(SEGMENTS), env=NO_SLIM),
        _r("r8-mirror-segmented", (8, 0, 1, 1, 0, 0, 0), 500, 8, "segmented", SWEEP_SEGMENT_APPLY | SWEEP_LIVE_SEGMENTS(SEGMENTS)),
        _r("r4-slim-frozen", (4, 0, 1, 2, 0, 0, 0), 400, 4, "frozen", SWEEP_FROZEN),
        _r("r16-walk32-frozen", (16, 0, 1, 0, 0, 0, 0), 1000, 16, "frozen", SWEEP_FROZEN, dict(narrow=0, **WALK)),
    ]
    return out


RECIPES = _recipes()
assert len({r.name for r in RECIPES}) == len(RECIPES)

# Compiled, resolvable, and asked for by no plan: key -> why.  tests/test_census_cases.py sweeps mvhdp_plan_probe over the whole domain
# and lets a key stand here only if no plan of that sweep asks for it.
NEVER_PLANNED = {}


# ---- the planner's word on a recipe (no device) ----
def plan_input(c, lists, known, flags, dbg, mix):
    """mvhdp_plan_input of the corpus, as tests/helpers.py::served_class builds it: list sizes unknown (the first sweep after
    build_counts) or known"""
    from mvtopicmodel_amd import _lib
    from tests.helpers import PLAN_REGS
    tot = sum(np.diff(np.asarray(o)) for o in c.doc_off)
    pi = _lib.PlanInputC()
    pi.num_topics, pi.num_modalities, pi.num_entities, pi.max_entity_tokens = c.K, c.M, c.D, int(tot.max())
    for q in range(5):
        pi.entities_longer_than[q] = int((tot > (64 << q)).sum())
    if known:
        for d, n in enumerate(lists):
            pi.entities_by_class[class_of_list(n)] += 1
            pi.tokens_by_list_rounds[min(16, (int(n) + 63) // 64 - 1)] += int(tot[d])
    pi.flags, pi.num_cus, pi.debug, pi.vectors_mix = flags, 256, int(dbg), int(mix)
    pi.trees_current = 1 if flags & SWEEP_FROZEN else 0
    for q in range(6):
        for f in range(3):
            pi.kernel_registers[q][f] = PLAN_REGS[q][f]
    return pi


def class_of_list(n):
    return 5 if n > 1024 else int(min(5, max(0, int(np.ceil(np.log2(max(n, 1) / 64.0))))))


def probe_tuning(tuning, env):
    """mvhdp_tuning as the recipe's handle has it; narrow = 2 tells the probe that the handle keeps the 12-bit image (it does wherever the
    image pays, unless MVHDP_SLIM=0 was set at create)"""
    from mvtopicmodel_amd import _lib
    t = _lib.TuningC()
    t.narrow = t.live16 = t.live_rows = t.live_overlap = -1
    for g in range(4):
        t.learnt_walk_step[g] = -1
    for k, v in tuning.items():
        if k in ("walk_theta", "tree_branch_share", "learnt_walk_step"):
            for i, x in enumerate(v):
                getattr(t, k)[i] = x
        else:
            setattr(t, k, v)
    if t.narrow == -1 and env.get("MVHDP_SLIM") != "0":
        t.narrow = 2
    return t


def keys_of_plan(po, K, live, dbg, mix, slim_handle, resolve):
    """{launched class: key} of a plan (mvhdp_plan_output): each class's walk / narrow, the sweep's live-rows form, debug, mix and K as
    the FastRequest mvhdp_launch_sweep_fast makes of them, through resolve (the header's rule); None where the rule refuses"""
    out = {}
    for q in range(6):
        if not po.class_used[q]:
            continue
        if not po.class_register_resident[q]:
            out[q] = (0, int(dbg), 0, 0, 0, 0, int(mix))
            continue
        narrow = po.class_narrow[q]
        live16 = int(bool(live) and narrow == 1)                 # (a live sweep is on the mirror only when it keeps it current: SweepPlan::live16)
        out[q] = resolve((1 << q, K, int(dbg), po.class_walk[q], narrow, po.live_rows, live16, int(mix), int(slim_handle)))
    return out
