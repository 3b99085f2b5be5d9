"""mvhdp_group_diagnostics: the diagnostics of a model sharded over document ranges equal those of one handle holding every entity.
In one process (2 and 4 members on one device) and across 2 and 4 rank processes over tests/native/fake_rccl.c (every rank a fresh
child process under its own time limit, as tests/test_gpu_group_ranks.py).  Integers exactly, doubles to 1e-12."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mvtopicmodel_amd import NativeGroup, NativeSampler
from mvtopicmodel_amd.java_init import init_assignments
from mvtopicmodel_amd.native import Hyper
from tests import diag_rank_worker as DW
from tests import rank_worker as W
from tests.helpers import make_native, shards_of, small_corpus
from tests.native_build import fake_rccl  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTS = ("codoc", "top_words", "top_counts", "nonzero", "num_rank1_docs", "num_nonzero_docs", "num_docs_at_proportions", "word_type_counts")


def _close(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), what
    f = np.isfinite(a)
    np.testing.assert_allclose(a[f], b[f], rtol=1e-12, atol=0, err_msg=what)


def assert_same(dg, d1):
    for f in INTS:
        assert np.array_equal(getattr(dg, f), getattr(d1, f)), f
    assert dg.num_tokens == d1.num_tokens
    _close(dg.sum_count_log_count, d1.sum_count_log_count, "sum_count_log_count")
    _close(dg.discr_weight_per_view, d1.discr_weight_per_view, "discr_weight_per_view")
    for name in d1.scores:
        _close(dg.scores[name], d1.scores[name], name)
        _close(dg.word_scores[name], d1.word_scores[name], name + " words")


@pytest.mark.parametrize("n", [2, 4])
def test_in_process_group_equals_the_single_handle(n):
    K, V = 60, [700, 90, 70]
    c = small_corpus(K, V, 200, [40, 5, 6], 98)
    hy = Hyper.defaults(K, V)
    z = init_assignments(K, c.doc_off, seed=4)
    one = make_native(c, hy, z)
    shards = [make_native(sub, hy, zs, doc_id_base=lo) for lo, sub, zs in shards_of(c, z, n)]
    with NativeGroup(shards) as g:
        g.build_counts()
        g.sweep(0, 13)
        one.sweep(0, 13)
        for m in range(c.M):
            assert np.array_equal(np.concatenate([s.get_assignments(m) for s in shards]), one.get_assignments(m))
        assert_same(g.diagnostics(num_top_words=20), one.diagnostics(num_top_words=20))
        assert_same(g.diagnostics(num_top_words=64), one.diagnostics(num_top_words=64))
        assert np.array_equal(shards[-1].discr_weights(), one.discr_weights())       # any member's
    for s in shards + [one]:
        s.close()


@pytest.mark.parametrize("nranks", [2, 4])
def test_rank_processes_equal_the_single_handle(tmp_path, fake_rccl, nranks):
    env = dict(os.environ)
    env["MVHDP_RCCL_LIB"] = fake_rccl
    env["FAKE_RCCL_TIMEOUT_MS"] = "20000"
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "diag_rank_worker.py"), str(tmp_path), str(r), str(nranks)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(nranks)]
    outs = []
    try:
        for p in procs:
            o, _ = p.communicate(timeout=240)
            outs.append(o)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{outs[r][-3000:]}"
    arrs = [dict(np.load(os.path.join(str(tmp_path), f"diag{r}.npz"))) for r in range(nranks)]
    c, z = W.corpus()
    with make_native(c, W.hyper("deferred"), z) as one:
        one.sweep(0, W.SEED)
        for m in range(c.M):
            assert np.array_equal(np.concatenate([a[f"z{m}"] for a in arrs]), one.get_assignments(m)), f"view {m}"
        d = one.diagnostics(num_top_words=DW.N_TOP)
    for a in arrs:                                           # every rank holds the whole model's diagnostics
        assert np.array_equal(a["codoc"], d.codoc) and np.array_equal(a["top_words"], d.top_words)
        assert np.array_equal(a["rank1"], d.num_rank1_docs) and np.array_equal(a["nonzero_docs"], d.num_nonzero_docs)
        assert np.array_equal(a["props"], d.num_docs_at_proportions) and np.array_equal(a["wtc"], d.word_type_counts)
        assert int(a["tokens"][0]) == d.num_tokens
        _close(a["scl"], d.sum_count_log_count, "scl")
        _close(a["per_view"], d.discr_weight_per_view, "per_view")
        for i, name in enumerate(d.scores):
            _close(a[f"score_{i}"], d.scores[name], name)
