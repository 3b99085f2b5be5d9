"""Cost of the topic diagnostics (mvhdp_diagnostics, num_top_words = 20) at full corpus size, next to one deferred sweep of the
same chain and, optionally, the numpy restatement (tests/diag_numpy.py) on the same state.

  python tools/diagnostics_timing.py [--workloads C2,C3,C4,C5] [--sweeps 2] [--reps 3] [--checker C2,C3] [--out FILE]

Per workload: the BASELINE corpus (mvtopicmodel_amd.synth.CONFIGS), assignments from java_init (the reference's addInstances rule),
`--sweeps` deferred sweeps first, then `--reps` calls of diagnostics().  diagnostics() is synchronous: its time is the wall time of
the call (device work, the transfers of its outputs and the host-side assembly of the score rows).  The sweep's time is what the
library measures with hipEvents on its stream (SweepStats.total_ms: trees + sweep + apply).  One JSON line per workload.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="C2,C3,C4,C5")
    ap.add_argument("--sweeps", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--checker", default="", help="workloads on which the numpy checker is timed too")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from mvtopicmodel_amd import NativeSampler, synth
    from mvtopicmodel_amd.java_init import init_assignments
    from mvtopicmodel_amd.native import Hyper
    lines = []
    for name in [w for w in a.workloads.split(",") if w]:
        t0 = time.perf_counter()
        c = synth.make_config(name)
        inactive, k_init = synth.config_inactive(name)
        z = init_assignments(k_init, c.doc_off, seed=1)
        hy = Hyper.defaults(c.K, c.V, inactive=inactive)
        if inactive is not None:
            hy.alpha[:, c.K] = 0.1
        s = NativeSampler(c.K, c.V)
        for m in range(c.M):
            s.set_corpus(m, c.doc_off[m], c.tokens[m])
            s.set_assignments(m, z[m])
        s.set_hyper(hy)
        s.build_counts()
        setup_s = time.perf_counter() - t0
        sweep_ms = []
        for it in range(a.sweeps):
            st = s.sweep(it, 1234)
            sweep_ms.append(st.total_ms)
        diag_ms = []
        for _ in range(a.reps):
            s.synchronize()
            t1 = time.perf_counter()
            d = s.diagnostics(num_top_words=20)
            diag_ms.append((time.perf_counter() - t1) * 1e3)
        rec = dict(workload=name, K=c.K, V=c.V, D=int(c.D), view0_tokens=int(len(c.tokens[0])), setup_s=round(setup_s, 1),
                   deferred_sweep_ms=[round(x, 3) for x in sweep_ms], diagnostics_ms=[round(x, 3) for x in diag_ms],
                   diagnostics_ms_min=round(min(diag_ms), 3), num_tokens=d.num_tokens)
        if name in a.checker.split(","):
            from tests import diag_numpy as dn
            nwk = [s.get_counts(m)[0] for m in range(c.M)]
            nk0 = s.get_counts(0)[1]
            alpha, _ = s.get_alpha()
            t2 = time.perf_counter()
            ref = dn.diagnostics(nwk, nk0, alpha[0], float(hy.gamma[0]), float(hy.alpha_sum[0]), float(hy.beta[0]),
                                 c.doc_off[0], c.tokens[0], s.get_assignments(0), 20)
            rec["checker_s"] = round(time.perf_counter() - t2, 2)
            rec["checker_codoc_equal"] = bool(np.array_equal(ref["codoc"], d.codoc))
        s.close()
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
