"""One rank of a multi-process run of MVHDP_SWEEP_SHARD_BIRTHS through mvhdp_group_create_rank, for
tests/test_gpu_shard_births_ranks.py: a FRESH process per rank, all on cuda:0, the collective being tests/native/fake_rccl.c
(MVHDP_RCCL_LIB).  Test infrastructure.

  python tests/shard_births_worker.py <workdir> <rank> <nranks> <single_wave 0|1>

Every rank builds the same model (topics 40-59 of 60 inactive), keeps its document shard, forms the group from the id rank 0 leaves in
<workdir>/uid, runs three LIVE | SHARD_BIRTHS sweeps and leaves <workdir>/rank<r>.npz (state after every sweep) + rank<r>.json.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, V, D, LAM, CSEED = 60, [500, 60], 400, [40, 6], 45
FIRST_INACTIVE = 40
SEED, SWEEPS = 5, 3


def model():
    """corpus, hyper-parameters and starting assignments (no token on an inactive topic)"""
    from mvtopicmodel_amd.native import Hyper
    from tests.helpers import make_oracle, small_corpus
    c = small_corpus(K, V, D, LAM, CSEED)
    inactive = np.zeros(K, dtype=np.uint8); inactive[FIRST_INACTIVE:] = 1
    hy = Hyper.defaults(K, V, inactive=inactive); hy.alpha[:, K] = 50.0
    o = make_oracle(c, hy)
    z = [o.get_assignments(m) for m in range(c.M)]
    for m in range(c.M):
        z[m][z[m] >= FIRST_INACTIVE] = 7
    o.close()
    return c, hy, z


def shard(c, hy, z, lo, hi, single_wave):
    from tests.helpers import make_native
    sub = c.slice_docs(lo, hi)
    s = make_native(sub, hy, [z[m][c.doc_off[m][lo]:c.doc_off[m][hi]] for m in range(c.M)], doc_id_base=lo)
    if single_wave:
        s.set_tuning(single_wave=1, live16=0, live_rows=1, force_primary=1)
    return s


def bounds(c, n):
    from mvtopicmodel_amd import synth
    return synth.shard_bounds(sum(np.diff(c.doc_off[m]) for m in range(c.M)), n)


def main():
    workdir, rank, nranks, single_wave = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
    from mvtopicmodel_amd import NativeGroup
    from mvtopicmodel_amd.native import SWEEP_LIVE, SWEEP_LIVE_SEGMENTS, SWEEP_SHARD_BIRTHS
    c, hy, z = model()
    lo, hi = bounds(c, nranks)[rank]
    s = shard(c, hy, z, lo, hi, single_wave)
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
    g.build_counts()                                      # (every replica: the counts of all shards)
    info = g.info()
    log = {"rank": rank, "ranks": int(info.ranks), "rccl": int(info.rccl), "rccl_version": int(info.rccl_version), "events": []}
    out = {}
    for it in range(SWEEPS):
        st = g.sweep(it, SEED, SWEEP_LIVE | SWEEP_SHARD_BIRTHS | SWEEP_LIVE_SEGMENTS(1))[0]
        log["events"].append({"sweep": it, "tokens": int(st.tokens), "activations": int(st.activations), "activated_topic": int(st.activated_topic),
                              "activated_modality": int(st.activated_modality), "activation_key": int(st.activation_key)})
        a, ina = s.get_alpha()
        out[f"s{it}_alpha"] = a; out[f"s{it}_inactive"] = ina
        for m in range(c.M):
            out[f"s{it}_z{m}"] = s.get_assignments(m)
            nwk, nk = s.get_counts(m)
            out[f"s{it}_nwk{m}"] = nwk; out[f"s{it}_nk{m}"] = nk
    np.savez(os.path.join(workdir, f"rank{rank}.npz"), **out)
    with open(os.path.join(workdir, f"rank{rank}.json"), "w") as f:
        json.dump(log, f)
    g.close()
    s.close()


if __name__ == "__main__":
    main()
