"""MVHDP_SWEEP_SHARD_BIRTHS across rank processes (mvhdp_group_create_rank, one process per GPU): 2 and 4 FRESH processes on cuda:0
over tests/native/fake_rccl.c (the real RCCL refuses two ranks on one device), each running tests/shard_births_worker.py.  Every rank
must hold the same replica after each sweep, give birth to more than one topic per exchange and keep births a prefix of the inactive
list; with one resident wave per rank the end state must be that of the same shards as one in-process group."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import shard_births_worker as W
from tests.native_build import fake_rccl  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, fake, nranks, single_wave, timeout=240):
    env = dict(os.environ, MVHDP_RCCL_LIB=fake, FAKE_RCCL_TIMEOUT_MS="20000")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "shard_births_worker.py"), str(tmp_path), str(r), str(nranks), str(single_wave)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(nranks)]
    outs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=timeout)
            outs.append(o)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()                                    # (the exact processes started here)
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and os.path.exists(os.path.join(str(tmp_path), f"rank{r}.json")), f"rank {r} failed:\n{o[-3000:]}"
    logs = [json.load(open(os.path.join(str(tmp_path), f"rank{r}.json"))) for r in range(nranks)]
    arrs = [dict(np.load(os.path.join(str(tmp_path), f"rank{r}.npz"))) for r in range(nranks)]
    assert all(lg["ranks"] == nranks and lg["rccl"] == 1 for lg in logs)
    return logs, arrs


def _check_invariants(c, logs, arrs):
    ina_before = np.zeros(W.K, dtype=np.uint8); ina_before[W.FIRST_INACTIVE:] = 1
    for it in range(W.SWEEPS):
        ev = [lg["events"][it] for lg in logs]
        assert all((e["activations"], e["activated_topic"], e["activated_modality"], e["activation_key"]) ==
                   (ev[0]["activations"], ev[0]["activated_topic"], ev[0]["activated_modality"], ev[0]["activation_key"]) for e in ev)
        al, ina = arrs[0][f"s{it}_alpha"], arrs[0][f"s{it}_inactive"]
        for a in arrs[1:]:
            assert np.array_equal(a[f"s{it}_alpha"], al) and np.array_equal(a[f"s{it}_inactive"], ina), f"sweep {it}: the replicas disagree"
        newly = np.flatnonzero(ina_before.astype(bool) & ~ina.astype(bool))
        assert newly.size == ev[0]["activations"]
        assert np.array_equal(newly, np.flatnonzero(ina_before)[:newly.size]), "births are not a prefix of the inactive list"
        assert all((al[:, t] == 50.0).sum() == 1 for t in newly)
        if it == 0:
            assert newly.size > 1, "one birth per exchange"
        z = [np.concatenate([a[f"s{it}_z{m}"] for a in arrs]) for m in range(c.M)]
        for m in range(c.M):
            assert not np.isin(z[m], np.flatnonzero(ina)).any(), "an assignment refers to a topic that is still inactive"
            want = np.zeros((c.V[m], c.K), dtype=np.int64)
            np.add.at(want, (c.tokens[m], z[m]), 1)
            for a in arrs:
                assert np.array_equal(a[f"s{it}_nwk{m}"].astype(np.int64), want) and np.array_equal(a[f"s{it}_nk{m}"].astype(np.int64), want.sum(axis=0))
        ina_before = ina
    assert not ina_before.any(), "not every topic was born within three sweeps"


@pytest.mark.parametrize("nranks", [2, 4])
def test_shard_births_across_ranks(tmp_path, fake_rccl, nranks):
    c, hy, z = W.model()
    logs, arrs = _run(tmp_path, fake_rccl, nranks, 0)
    _check_invariants(c, logs, arrs)


@pytest.mark.parametrize("nranks", [2, 4])
def test_one_wave_ranks_equal_the_same_shards_as_one_process_group(tmp_path, fake_rccl, nranks):
    c, hy, z = W.model()
    logs, arrs = _run(tmp_path, fake_rccl, nranks, 1)
    _check_invariants(c, logs, arrs)
    # every rank has exited: the same shards as members of one in-process group
    from mvtopicmodel_amd import NativeGroup
    from mvtopicmodel_amd.native import SWEEP_LIVE, SWEEP_LIVE_SEGMENTS, SWEEP_SHARD_BIRTHS
    shards = [W.shard(c, hy, z, lo, hi, 1) for lo, hi in W.bounds(c, nranks)]
    with NativeGroup(shards) as g:
        g.build_counts()
        for it in range(W.SWEEPS):
            g.sweep(it, W.SEED, SWEEP_LIVE | SWEEP_SHARD_BIRTHS | SWEEP_LIVE_SEGMENTS(1))
    last = W.SWEEPS - 1
    for r, s in enumerate(shards):
        a, ina = s.get_alpha()
        assert np.array_equal(a, arrs[r][f"s{last}_alpha"]) and np.array_equal(ina, arrs[r][f"s{last}_inactive"])
        for m in range(c.M):
            assert np.array_equal(s.get_assignments(m), arrs[r][f"s{last}_z{m}"]), f"rank {r}: z differs in view {m}"
            nwk, nk = s.get_counts(m)
            assert np.array_equal(nwk, arrs[r][f"s{last}_nwk{m}"]) and np.array_equal(nk, arrs[r][f"s{last}_nk{m}"])
    for s in shards:
        s.close()
