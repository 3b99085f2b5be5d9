"""One rank of a multi-process mvhdp_group_diagnostics run, for tests/test_gpu_diagnostics_group.py: a FRESH process per rank, all on
cuda:0, the collective being tests/native/fake_rccl.c (MVHDP_RCCL_LIB).  Test infrastructure.

  python tests/diag_rank_worker.py <workdir> <rank> <nranks>

Every rank builds the corpus of tests/rank_worker.py, keeps its document shard, forms the group from the id rank 0 leaves in
<workdir>/uid, runs one group sweep and the group's diagnostics, and leaves <workdir>/diag<r>.npz.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import rank_worker as W  # noqa: E402

N_TOP = 20


def main():
    workdir, rank, nranks = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    from mvtopicmodel_amd import NativeGroup, NativeSampler, synth
    c, z = W.corpus()
    hy = W.hyper("deferred")
    tot = sum(np.diff(c.doc_off[m]) for m in range(c.M))
    lo, hi = synth.shard_bounds(tot, nranks)[rank]
    sub = c.slice_docs(lo, hi)
    s = NativeSampler(W.K, W.V, device=0, doc_id_base=lo)
    for m in range(c.M):
        s.set_corpus(m, sub.doc_off[m], sub.tokens[m])
        s.set_assignments(m, z[m][c.doc_off[m][lo]:c.doc_off[m][hi]])
    s.set_hyper(hy)
    s.build_counts()
    uid_path = os.path.join(workdir, "uid")
    if rank == 0:
        uid = NativeGroup.unique_id()
        with open(uid_path + ".tmp", "wb") as f:
            f.write(uid)
        os.rename(uid_path + ".tmp", uid_path)
    else:
        t0 = time.time()
        while not os.path.exists(uid_path):
            if time.time() - t0 > 120:
                raise SystemExit("no id from rank 0")
            time.sleep(0.02)
        uid = open(uid_path, "rb").read()
    g = NativeGroup.from_rank(s, uid, rank, nranks)
    g.build_counts()                                       # the whole model's counts on every replica (collective)
    g.sweep(0, W.SEED)
    d = g.diagnostics(num_top_words=N_TOP)
    out = {f"score_{i}": d.scores[n] for i, n in enumerate(d.scores)}
    out.update(codoc=d.codoc, top_words=d.top_words, rank1=d.num_rank1_docs, nonzero_docs=d.num_nonzero_docs,
               props=d.num_docs_at_proportions, scl=d.sum_count_log_count, wtc=d.word_type_counts, tokens=np.array([d.num_tokens]),
               per_view=d.discr_weight_per_view)
    for m in range(c.M):
        out[f"z{m}"] = s.get_assignments(m)
    np.savez(os.path.join(workdir, f"diag{rank}.npz"), **out)
    g.close()
    s.close()


if __name__ == "__main__":
    main()
