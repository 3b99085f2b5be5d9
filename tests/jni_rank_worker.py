"""One rank of a two-process run THROUGH THE JNI SHIM (nGroupUniqueId / nGroupCreateRank / nGroupSweep ...), for
tests/test_gpu_jni.py: a fresh process per rank, all on device 0, the collective being tests/native/fake_rccl.c (MVHDP_RCCL_LIB).
Test infrastructure.

  python tests/jni_rank_worker.py <workdir> <rank> <nranks> <the shim + fake JVM library tests/jni_harness.py built>

Every rank builds the same synthetic corpus, keeps its document shard, forms the group from the id rank 0 leaves in <workdir>/uid,
runs two deferred sweeps, then forms a second group of the same sharding through the Python binding (the id in <workdir>/uid_binding)
for the statistic whose value depends on the sharding, and leaves <workdir>/rank<r>.npz + rank<r>.json."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, V, D, LAM, CSEED = 48, [700, 90, 70], 260, [40, 5, 6], 97
SEED = 11


def corpus():
    from mvtopicmodel_amd import synth
    from mvtopicmodel_amd.java_init import init_assignments
    c = synth.generate(K, V, D, LAM, CSEED, chunk_docs=4096)
    return c, init_assignments(K, c.doc_off, seed=1)


def hyper():
    from mvtopicmodel_amd.native import Hyper
    return Hyper.defaults(K, V)


def shared_id(workdir, name, rank, make):
    """the id rank 0 makes, left in <workdir>/<name> for the other ranks"""
    path = os.path.join(workdir, name)
    if rank == 0:
        uid = make()
        with open(path + ".tmp", "wb") as f:
            f.write(uid)
        os.rename(path + ".tmp", path)
        return uid
    t0 = time.time()
    while not os.path.exists(path):
        if time.time() - t0 > 120:
            raise SystemExit("no id from rank 0")
        time.sleep(0.02)
    return open(path, "rb").read()


def main():
    workdir, rank, nranks, lib = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    from mvtopicmodel_amd import _lib, synth
    from tests import jni_harness as H
    _lib.load_library()
    jvm = H.Jvm(lib)
    c, z = corpus()
    hy = hyper()
    tot = sum(np.diff(c.doc_off[m]) for m in range(c.M))
    lo, hi = synth.shard_bounds(tot, nranks)[rank]
    sub = c.slice_docs(lo, hi)
    s = H.JniSampler(jvm, K, V, 0, lo)
    for m in range(c.M):
        s.setCorpus(m, sub.doc_off[m], sub.tokens[m])
        s.setAssignments(m, z[m][c.doc_off[m][lo]:c.doc_off[m][hi]])
    s.setHyper(hy.alpha, hy.alpha_sum, hy.beta, hy.beta_sum, hy.gamma, hy.p_a, hy.p_b, None)
    s.buildCounts()
    uid = shared_id(workdir, "uid", rank, lambda: H.JniGroup.uniqueId(jvm).tobytes())
    assert len(uid) == 128
    uid = np.frombuffer(uid, dtype=np.int8)
    g = H.JniGroup.ofRank(jvm, s, uid, rank, nranks)
    g.buildCounts()
    log = {"rank": rank, "sweeps": []}
    for it in range(2):
        st = g.sweep(it, SEED, 0)[0]
        log["sweeps"].append({"tokens": st.tokens, "changed": st.changed, "exchange_ms": st.totalMs})
    out = {"ll": g.modelLogLikelihood(c.M)}
    for m in range(c.M):
        out[f"z{m}"] = s.getAssignments(m, len(sub.tokens[m]))
        out[f"nwk{m}"], out[f"nk{m}"] = s.getCounts(m, V[m], K)
    log["ledger_checked"] = len(jvm.log)
    g.close()
    s.close()
    # the same statistic through the Python binding, as the same rank of a second group over the state the sweeps left: across
    # processes the ranks' document sums are added in rank order (equal to a single handle's to rounding only), so the exact
    # reference for modelLogLikelihood of a rank is the binding's group of the same sharding, not the single handle
    from mvtopicmodel_amd import NativeGroup, NativeSampler
    b = NativeSampler(K, V, device=0, doc_id_base=lo)
    for m in range(c.M):
        b.set_corpus(m, sub.doc_off[m], sub.tokens[m])
        b.set_assignments(m, out[f"z{m}"])
    b.set_hyper(hy)
    b.build_counts()
    gb = NativeGroup.from_rank(b, shared_id(workdir, "uid_binding", rank, NativeGroup.unique_id), rank, nranks)
    gb.build_counts()
    out["ll_binding"] = gb.model_log_likelihood()
    gb.close()
    b.close()
    np.savez(os.path.join(workdir, f"rank{rank}.npz"), **out)
    with open(os.path.join(workdir, f"rank{rank}.json"), "w") as f:
        json.dump(log, f)


if __name__ == "__main__":
    main()
