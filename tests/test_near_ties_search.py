"""The near-tie generator (tests/near_ties.py) with the oracle alone: what it returns is deterministic, every flip is
a pair of adjacent doubles with different outcomes, and the fixed searches the GPU tests run meet the quotas those tests
rely on -- so that they cannot pass for want of cases."""
import numpy as np
import pytest

from tests import near_ties as nt
from tests.helpers import served_class

_built = {}


def _deferred(name):
    """the flips of a deferred case, searched once for all the tests of this file"""
    if name not in _built:
        _built[name] = nt.deferred_flips(name)
    return _built[name]


def _check_flips(ev, flips):
    for f in flips:
        assert f.lo < f.hi and np.nextafter(f.lo, f.hi) == f.hi, f
        ev.seed = f.seed
        a, b = ev.run(f.param, f.lo), ev.run(f.param, f.hi)
        assert a.key != b.key, f
        assert a.stats["aborted_docs"] == 0 and b.stats["aborted_docs"] == 0


def test_search_is_deterministic():
    _, one = _deferred("small")
    _, two = nt.deferred_flips("small")
    assert one == two and len(one) >= 24
    form = nt.LIVE_FORMS[1]
    assert nt.live_flips(form)[1] == nt.live_flips(form)[1]


@pytest.mark.parametrize("name", list(nt.DEFERRED_PLAN))
def test_deferred_searches_meet_their_quotas(name):
    ev, flips = _deferred(name)
    forced = nt.DEFERRED_PLAN[name][1]
    for R in forced:
        # the planner runs the variant named and lets it serve every entity; no narrower variant could hold any of the lists
        assert served_class(ev.case, R) == R.bit_length() - 1, f"force_primary {R} is not what would serve {name}"
        assert all(64 * (R // 2) < n <= 64 * R for n in ev.case.list_lengths())
    _check_flips(ev, flips)
    nt.check_deferred_quotas(flips, forced, wide=name.startswith("wide"))
    if name.startswith("wide"):
        assert ev.case.K >= 1000 and min(np.diff(ev.case.doc_off[0])) > 1000
    if name == "wide16":
        assert ev.case.M == 8


def test_every_register_variant_and_one_to_eight_views_have_a_case():
    assert sorted(R for _, forced in nt.DEFERRED_PLAN.values() for R in forced) == [1, 1, 2, 4, 8, 16]
    assert {mk().M for mk, _ in nt.DEFERRED_PLAN.values()} >= {1, 2, 8}


@pytest.mark.parametrize("form", nt.LIVE_FORMS, ids=lambda f: "rows%d-cell16_%d" % (f["rows"], f["cell16"]))
def test_live_searches_meet_their_quotas(form):
    ev, flips = nt.live_flips(form)
    assert ev.case.hy.inactive is None             # (what the classification of a live flip rests on)
    _check_flips(ev, flips)
    nt.check_live_quotas(flips)


@pytest.mark.parametrize("name", ["single", "small"])
def test_ladders_keep_their_rungs(name):
    """a rung at which the oracle abandons an entity is left out by the generator: at most one in twenty"""
    ev, flips = _deferred(name)
    dropped, kept = [0], 0
    for f in flips:
        rungs = list(nt.ladder(ev, f, nt.THIN_JS, dropped))
        kept += len(rungs)
        assert [r.x for r in rungs[:2]] == [f.lo, f.hi]
        xs = [r.x for r in rungs]
        assert len(set(xs)) == len(xs) and min(xs) > 0
        assert abs(rungs[-1].x - f.hi) == 2.0 ** nt.J_MAX * (f.hi - f.lo)
    assert dropped[0] * 20 <= kept + dropped[0]
