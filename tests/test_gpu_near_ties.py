"""The sweep's decisions at constructed near-ties (tests/near_ties.py): hyper-parameter values one ulp either side of a
point where the oracle's outcome changes, and ladders of values 2^j ulp away from it (j = 0 .. 40), which move one
comparison's margin from a few fp64 ulps of the total through the certified tolerance of the DPP scan
((4 * S_used + 16) * 2^-53) and the fp32 screen's (2^-17) to clearly outside both.  Every kernel flavour must give the
oracle's integers at every rung; at the flip itself the comparison is closer than any tolerance, so the sequential
left-to-right sum must have decided it (exact_fallbacks >= 1), and far from it the counter must be able to stay zero.

No debug rows and no trace are asked of the product: that would select the flavour without the fp32 screen."""
import numpy as np
import pytest

from tests import near_ties as nt
from tests.helpers import (assert_same_state, check_fallback_counters, every_rung, make_native, rung_name, run_deferred_ladders,
                           same_statistics, wide_rungs)
from mvtopicmodel_amd.native import SWEEP_LIVE, SWEEP_LIVE_SEGMENTS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(nt.DEFERRED_PLAN))
def test_deferred_sweeps_at_near_ties(name):
    ev, flips = nt.deferred_flips(name)
    forced = nt.DEFERRED_PLAN[name][1]
    nt.check_deferred_quotas(flips, forced, wide=name.startswith("wide"))
    wide = name.startswith("wide")
    long_lists = ev.case.max_list() > 64                     # (beyond one round the exact chain and the generic kernel get fewer rungs: helpers.wide_rungs)
    fb, kept, dropped = run_deferred_ladders(ev, flips, forced, nt.WIDE_JS if wide else nt.THIN_JS, wide_rungs if long_lists else every_rung)
    print(f"near-ties {name}: {len(flips)} flips, {kept} rungs ({dropped} dropped), {sum(len(v) for v in fb.values())} sweeps")
    check_fallback_counters(flips, fb)


@pytest.mark.parametrize("form", nt.LIVE_FORMS, ids=lambda f: "rows%d-live16_%d" % (f["rows"], f["cell16"]))
def test_one_wave_live_sweeps_at_near_ties(form):
    """The live path with one resident wavefront against Oracle.sweep_live_seq: the count branch as above, the tree branch
    sampling the word's live row in fp32 (rows = 1) -- where an fp32 operation contracted or ordered otherwise than the
    oracle restates it would show."""
    ev, flips = nt.live_flips(form)
    nt.check_live_quotas(flips)
    case = ev.case
    s = make_native(case, case.hy, case.z0)
    s.set_tuning(live16=form["cell16"], single_wave=1, live_rows=form["rows"], force_primary=1)
    dropped, kept = [0], 0
    for fi, f in enumerate(flips):
        for rung in nt.ladder(ev, f, nt.THIN_JS, dropped):
            kept += 1
            where = f"live {form} {f.param} = {float(rung.x).hex()} (flip {fi} kind {f.kind}, {rung_name(rung)}) seed {f.seed}"
            ev.prepare(s, ev.hyper_at(f.param, rung.x), s.set_hyper)
            rs = s.sweep(ev.sweep_idx, f.seed, flags=SWEEP_LIVE | SWEEP_LIVE_SEGMENTS(1))
            same_statistics(rs, rung.stats, where)
            try:
                assert_same_state(ev.o, s, case.M)
            except AssertionError as e:
                raise AssertionError(f"{where}: {e}") from None
    s.close()
    assert dropped[0] * 20 <= kept + dropped[0]
    print(f"near-ties live {form}: {len(flips)} flips, {kept} rungs ({dropped[0]} dropped), {kept} sweeps")
