"""Oracle parity where the magnitudes leave the range every other test runs in: hyper-parameters from 1e-8 to 100, ten
decades of alpha inside one scan, counts beyond 2^24 (where (float)g of the fp32 screen rounds and n_k + beta_sum
nears 2^30), and a new-topic mass that is negligible or dominates the total.  Every register variant, the generic
kernel and the exact chain must give the oracle's integers for three sweeps; the near-tie ladders of
tests/test_gpu_near_ties.py run on one planted-count corpus and one ten-decade-alpha corpus as well."""
import numpy as np
import pytest

from tests import near_ties as nt
from tests.helpers import (After, assert_same_state, check_fallback_counters, every_rung, make_native, run_deferred_ladders,
                           same_statistics, served_class, wide_rungs)
from mvtopicmodel_amd.native import SWEEP_EXACT_CHAIN, SWEEP_GENERIC_KERNEL

pytestmark = pytest.mark.gpu

PLANT = 20_000_000
K, V = 1000, [300, 60]
FORCED = (1, 4, 16)


def _case(n_inactive=0):
    """One entity whose list needs the 16-round variant, three for the 4-round one, eight for the 1-round one: with
    force_primary 1, 4, 16 that variant is the primary and serves its share, longer lists going to wider classes."""
    rng = np.random.RandomState(21)
    lens0 = np.concatenate([[800], 440 + rng.randint(0, 30, 3), np.maximum(rng.poisson(50, 8), 1)])
    lens1 = np.maximum(rng.poisson(6, 12), 1)
    case = nt.make_case("extreme", K, V, [lens0, lens1], 21, [K] + [270] * 3 + [30] * 8, n_inactive=n_inactive)
    n = case.list_lengths()
    assert n[0] > 512 and all(128 < x <= 256 for x in n[1:4]) and all(x <= 64 for x in n[4:])
    return case


def _set(hy, alpha=None, beta=None, gamma=None):
    if alpha is not None:
        hy.alpha[:] = alpha
        hy.alpha_sum[:] = hy.alpha[:, :K].sum(axis=1)
    if beta is not None:
        hy.beta[:] = beta
        hy.beta_sum[:] = hy.beta * np.array(V)
    if gamma is not None:
        hy.gamma[:] = gamma


SETTINGS = {
    "beta1e-6_alpha1e-8": dict(beta=1e-6, alpha=1e-8),
    "alpha50_gamma100": dict(alpha=50.0, gamma=100.0),
    "gamma1e-3_beta5": dict(gamma=1e-3, beta=5.0),
    "alpha_ten_decades": dict(alpha=np.logspace(-8, 2, K + 1)),
}


def _parity_three_sweeps(case, plant, seed):
    ev = nt.Evaluator(case, seed, plant=plant)
    o, hy, M = ev.o, case.hy, case.M
    ev.prepare(o, hy, lambda h: o.set_hyper(h.alpha, h.alpha_sum, h.beta, h.beta_sum, h.gamma, h.p_a, h.p_b, h.inactive))
    if plant:
        assert max(int(o.get_counts(m)[1].max()) for m in range(M)) > (1 << 24)
    want = []
    for it in range(3):
        st = o.sweep(it, seed)["stats"]
        assert st["aborted_docs"] == 0
        want.append((st, After(o, M), o.get_alpha(), o.get_inactive()))
    for force in (0,) + FORCED:
        if force:
            assert served_class(case, force, every=False) == force.bit_length() - 1, f"force_primary {force} is not what the planner runs"
        s = make_native(case, hy, case.z0)
        s.set_tuning(force_primary=force)
        for kernel in ((0, SWEEP_GENERIC_KERNEL) if force == 0 else (0,)):
            for chain in (0, SWEEP_EXACT_CHAIN):
                ev.prepare(s, hy, s.set_hyper)
                for it in range(3):
                    where = f"force_primary {force} flags {kernel | chain:#x} sweep {it}"
                    rs = s.sweep(it, seed, flags=kernel | chain)
                    st, after, alpha, inactive = want[it]
                    same_statistics(rs, st, where)
                    try:
                        assert_same_state(after, s, M)
                    except AssertionError as e:
                        raise AssertionError(f"{where}: {e}") from None
                    a, ina = s.get_alpha()
                    assert np.array_equal(a, alpha) and np.array_equal(ina, inactive), where
        s.close()
    return want


@pytest.mark.parametrize("plant", [0, PLANT], ids=["counted", "planted"])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_extreme_hyper_parameters(setting, plant):
    case = _case()
    _set(case.hy, **SETTINGS[setting])
    want = _parity_three_sweeps(case, plant, 31)
    assert sum(w[0]["changed"] for w in want) > 0


@pytest.mark.parametrize("alpha_new", [1e-6, 1e4])
def test_truncated_hdp_with_a_negligible_and_a_dominant_new_topic_mass(alpha_new):
    case = _case(n_inactive=3)
    case.hy.alpha[:, K] = alpha_new
    want = _parity_three_sweeps(case, 0, 37)
    if alpha_new > 1:                                            # the new-topic branch is taken, and topics are born
        assert want[0][0]["new_mass_cnt"] > 0 and want[0][0]["activated_topic"] >= 0


_LADDER_CAP = {"A": 4, "B": 4, "C": 6, "D": 1}


@pytest.mark.parametrize("name,R", [("mid4", 4), ("wide16", 16)])
@pytest.mark.parametrize("which", ["planted", "alpha_ten_decades"])
def test_near_tie_ladders_at_extreme_magnitudes(which, name, R):
    """on the cases whose entities the 4-round resp. the 16-round variant serves (tests/near_ties.py::DEFERRED_PLAN)"""
    case = nt.DEFERRED_PLAN[name][0]()
    plant = 0
    if which == "planted":
        plant = PLANT
    else:
        aK = case.hy.alpha[:, case.K].copy()                     # (the new-topic weight stays: kind A needs a mass that can be met)
        case.hy.alpha[:] = np.logspace(-8, 2, case.K + 1)
        case.hy.alpha[:, case.K] = aK
        case.hy.alpha_sum[:] = case.hy.alpha[:, :case.K].sum(axis=1)
    ev, flips = nt.deferred_flips(name, plant=plant, case=case, cap=_LADDER_CAP)
    n = {k: sum(f.kind == k for f in flips) for k in "ABC"}
    assert min(n.values()) >= 3, n
    wide = name.startswith("wide")
    fb, kept, dropped = run_deferred_ladders(ev, flips, [R], nt.WIDE_JS if wide else nt.THIN_JS, wide_rungs if wide else every_rung,
                                             others=("default",))
    print(f"near-ties {which} {name}: {len(flips)} flips, {kept} rungs ({dropped} dropped), {sum(len(v) for v in fb.values())} sweeps")
    check_fallback_counters(flips, fb)
