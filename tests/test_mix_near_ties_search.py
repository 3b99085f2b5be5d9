"""The near-tie search under the useVectorsLambda mix (tests/mix_near_ties.py) on the CPU: the fixed searches yield flips that ARE
flips -- adjacent doubles, different assignments, the first token that differs in view 0 --, of the kinds each case promises, and
the restatement itself abandons no more than 1 rung in 20 of their ladders (the cap the GPU test applies)."""
import numpy as np
import pytest

from tests import mix_near_ties


@pytest.mark.parametrize("name", sorted(mix_near_ties.PLAN))
def test_flips_are_flips(name):
    ev, flips, forced = mix_near_ties.flips_of(name)
    mix_near_ties.check_quotas(name, flips)
    kept = dropped = 0
    for f in flips:
        assert float(np.nextafter(f.lo, f.hi)) == f.hi
        ev.seed = f.seed
        a, b = ev.run(f.param, f.lo), ev.run(f.param, f.hi)
        assert a.key != b.key and f.token[1] == 0
        if f.param[0] == "lam":
            assert 0.0 < f.lo < f.hi < 1.0
        k, d = mix_near_ties.ladder_kept(ev, f)
        kept += k; dropped += d
    assert dropped * 20 <= kept + dropped, f"{dropped} rungs of {kept + dropped} abandoned by the restatement"
