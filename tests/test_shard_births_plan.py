"""MVHDP_SWEEP_SHARD_BIRTHS in the sweep's planner (mvhdp_plan_probe, no GPU): the flag goes with LIVE -- a document shard's
NO_APPLY live sweep gives birth chunk by chunk in the live-rows form -- and is refused without LIVE, with FROZEN and with ONLY_SEGMENT."""
from mvtopicmodel_amd.native import (SWEEP_FROZEN, SWEEP_LIVE, SWEEP_LIVE_SEGMENTS, SWEEP_NO_APPLY, SWEEP_ONLY_SEGMENT,
                                     SWEEP_SHARD_BIRTHS)
from tests.test_plan import probe

INVALID_ARG = -1


def test_shard_births_flag_in_the_plan():
    for flags in (SWEEP_LIVE | SWEEP_NO_APPLY | SWEEP_SHARD_BIRTHS, SWEEP_LIVE | SWEEP_SHARD_BIRTHS,
                  SWEEP_LIVE | SWEEP_NO_APPLY | SWEEP_SHARD_BIRTHS | SWEEP_LIVE_SEGMENTS(2)):
        po = probe(K=60, M=2, D=400, mdt=60, longer=(0, 0, 0, 0, 0), flags=flags, inactive=1)
        assert po.status == 0 and po.live_rows == 1, flags
    for flags in (SWEEP_NO_APPLY | SWEEP_SHARD_BIRTHS, SWEEP_SHARD_BIRTHS, SWEEP_LIVE | SWEEP_FROZEN | SWEEP_SHARD_BIRTHS,
                  SWEEP_LIVE | SWEEP_NO_APPLY | SWEEP_SHARD_BIRTHS | SWEEP_LIVE_SEGMENTS(2) | SWEEP_ONLY_SEGMENT(1)):
        assert probe(K=60, M=2, D=400, mdt=60, longer=(0, 0, 0, 0, 0), flags=flags, inactive=1).status == INVALID_ARG, flags
