"""Cost of mvhdp_predict_items / mvhdp_score_items at C4 on the state after the benchmark's window: the random start of bench.py, 25
deferred sweeps, then three calls, each beside the path a user has without them.  Writes a markdown report (default profiles/xview.md).

  python tools/xview_timing.py [--workload C4] [--docs D] [--sweeps 25] [--out profiles/xview.md] [--no-profile]

  - predict_items(m = 1, n = 20) for every entity            (V_1 = 5000)
  - predict_items(m = 0, n = 20) for the first 10 000        (V_0 = 50 000)
  - score_items for 10^6 pairs of view 1 (one pair an entity, a type it holds where it holds one)
Wall times are host clocks around the synchronous call: three calls, the median of the last two.  The baseline is theta fetched with
doc_topic_proportions, then numpy's dgemm theta . phi^T and argpartition (or a comparison count per pair) on the host's threads, on a
slice of the entities (--baseline-entities), scaled to the call's entity count by the ratio -- it is linear in it.  The kernels' own
times come from a child run under `rocprofv3 --kernel-trace --stats`, the counters of the score kernel from another under
`rocprofv3 --pmc` (never together with a trace); both on a 50 000-entity model of the same shape, predicting view 1.  A child that
fails or runs into its time limit ends the profiling: its process group is killed and nothing more is started on the GPU."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import SEED, ChildFailed, profiled, resource_usage, timed, trained_sampler, weights_without  # noqa: E402

N_TOP = 20
MI355X_CUS, MI355X_MAX_GHZ = 256, 2.4
COUNTERS = ["SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_LDS_BANK_CONFLICT", "SQ_WAIT_INST_ANY", "SQ_INSTS_VALU", "SQ_INSTS_LDS"]
CHILD_DOCS = 50000
KERNELS = r"xview_\w+|doc_topic_prop_kernel"


def held_pairs(corpus, m, D, V):
    """one pair an entity: the first type of its view-m span, or type d mod V where it has none"""
    off, tok = corpus.doc_off[m], corpus.tokens[m]
    ent = np.arange(D, dtype=np.int64)
    has = off[1:D + 1] > off[:D]
    item = (ent % V).astype(np.int32)
    item[has] = tok[off[:D][has]]
    return ent, item


def host_path(s, hy, corpus, m, w, n_ent, pairs=None):
    """the path without the calls, on entities [0, n_ent): (ms for theta's round trip, ms for the rest)"""
    t0 = time.perf_counter()
    theta = s.doc_topic_proportions(w, 0, n_ent)
    t1 = time.perf_counter()
    nwk, nk = s.get_counts(m)
    phi = (nwk + hy.beta[m]) / (nk + hy.beta_sum[m])
    if hy.inactive is not None:
        phi[:, hy.inactive != 0] = 0.0
    S = theta @ phi.T
    off, tok = corpus.doc_off[m], corpus.tokens[m]
    rows = np.repeat(np.arange(n_ent), np.diff(off[:n_ent + 1]))
    if pairs is None:
        S[rows, tok[:off[n_ent]]] = -1.0                                     # the types an entity holds are not listed
        top = np.argpartition(-S, N_TOP - 1, axis=1)[:, :N_TOP]
        order = np.argsort(-np.take_along_axis(S, top, 1), axis=1, kind="stable")
        np.take_along_axis(top, order, 1)
    else:
        ent, item = pairs
        q = S[ent, item].copy()
        S[rows, tok[:off[n_ent]]] = -1.0
        (S[ent] > q[:, None]).sum(1)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C4")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--sweeps", type=int, default=25)
    ap.add_argument("--baseline-entities", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xview.md"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help="(internal) one predict_items call of view 1, for the profiler")
    args = ap.parse_args()
    if args.child:
        s = trained_sampler(args.workload, CHILD_DOCS, 2)[0]
        s.predict_items(1 if s.M > 1 else 0, weights_without(s.M, 1 if s.M > 1 else 0), N_TOP)
        s.close()
        return
    s, hy, corpus, D, _ = trained_sampler(args.workload, args.docs, args.sweeps)
    print(f"{args.sweeps} sweeps done", file=sys.stderr, flush=True)
    K, V, M = s.K, s.V, s.M
    m1 = 1 if M > 1 else 0
    nb = min(args.baseline_entities, D)
    lines = ["# mvhdp_predict_items / mvhdp_score_items: timings", "",
             f"Written by tools/xview_timing.py.  Workload {args.workload}" + (f" cut to {args.docs} entities" if args.docs else "") +
             f": K = {K}, V = {V}, {D} entities; the random start of bench.py, then {args.sweeps} deferred sweeps (seed {SEED}).",
             "Wall times: host clock around the synchronous call, the median of 2 calls after 1.  Baseline: theta through doc_topic_proportions, "
             f"then numpy (dgemm, argpartition / comparison counts) on the host's threads (OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}), "
             f"measured on the first {nb} entities (view 0: {min(nb, 2000)}) and scaled by the entity count.", ""]

    def report(name, n_ent, f, base, n_base, work):
        first, med, r = timed(f)
        th_ms, rest_ms = base
        scale = n_ent / n_base
        lines.append(f"- {name}: {med:.1f} ms a call (first call {first:.1f} ms) = {work / med / 1e6:.2f} G fp64 FMA/s over the whole call; "
                     f"host path: {th_ms * scale:.0f} ms for theta's round trip + {rest_ms * scale:.0f} ms of numpy = {(th_ms + rest_ms) * scale / med:.1f} x the call "
                     f"(measured on {n_base} entities: {th_ms:.0f} + {rest_ms:.0f} ms)")
        print(lines[-1], file=sys.stderr, flush=True)
        return r

    w1, w0 = weights_without(M, m1), weights_without(M, 0)
    report(f"predict_items(m = {m1}, n = {N_TOP}), {D} entities, V = {V[m1]}", D, lambda: s.predict_items(m1, w1, N_TOP),
           host_path(s, hy, corpus, m1, w1, nb), nb, D * V[m1] * K)
    n0 = min(10000, D)
    nb0 = min(nb, n0, 2000)                                                  # (a 2000 x 50 000 fp64 block and its copies: 2.4 GB)
    report(f"predict_items(m = 0, n = {N_TOP}), {n0} entities, V = {V[0]}", n0, lambda: s.predict_items(0, w0, N_TOP, 0, n0),
           host_path(s, hy, corpus, 0, w0, nb0), nb0, n0 * V[0] * K)
    ent, item = held_pairs(corpus, m1, D, V[m1])
    r = report(f"score_items(m = {m1}), {D} pairs on {D} entities", D, lambda: s.score_items(m1, w1, ent, item),
               host_path(s, hy, corpus, m1, w1, nb, (ent[:nb], item[:nb])), nb, D * V[m1] * K)
    lines += [f"- those pairs: mean log score {r.mean_log_score():.4f}, recall@{N_TOP} {r.recall_at(N_TOP):.4f}, MRR {r.mrr():.4f} "
              f"(a uniform guess over {V[m1]} types: log score {-np.log(V[m1]):.4f})", ""]
    s.close()
    lines += ["## the score kernel as compiled", ""] + [f"- {a}: {b}" for _, _, got in resource_usage("mvhdp_xview.hip", "xview_score_kernel") for a, b in got.items()] + [""]
    if not args.no_profile:
        lines += [f"## the kernels of one predict_items(m = {m1}, n = {N_TOP}) call on {CHILD_DOCS} entities (child runs of their own, a model trained for 2 sweeps)", ""]
        ks = pm = None
        try:
            print("wall times taken; the kernel trace", file=sys.stderr, flush=True)
            ks = profiled(__file__, ["--workload", args.workload], KERNELS)
            print("the counter pass", file=sys.stderr, flush=True)
            pm = profiled(__file__, ["--workload", args.workload], "xview_score_kernel", mode="pmc", counters=COUNTERS)
        except ChildFailed as e:
            lines += [f"- {e}; no further run was started", ""]
        score_ms = None
        if ks:
            total = sum(ms for _, ms in ks.values())
            for name, (calls, ms) in sorted(ks.items(), key=lambda e: -e[1][1]):
                lines.append(f"- {name}: {ms:.2f} ms over {calls} launch(es), {100 * ms / total:.0f} % of the call's kernel time")
            score_ms = ks.get("xview_score_kernel", (0, None))[1]
            if score_ms:
                fma = CHILD_DOCS * V[m1] * K
                sel = sum(ms for n, (_, ms) in ks.items() if n.startswith("xview_") and n not in ("xview_score_kernel", "xview_phi_kernel"))
                lines += [f"- xview_score_kernel: {fma} fp64 FMA in {score_ms:.2f} ms = {fma / score_ms / 1e9:.2f} T FMA/s ({2 * fma / score_ms / 1e9:.2f} TFLOP/s)",
                          f"- the selection (mark, select, order): {sel:.2f} ms = {100 * sel / total:.0f} % of the call's kernel time"]
            lines.append("")
        else:
            lines += ["- no kernel trace (rocprofv3 is not installed, gave no kernel rows, or the run failed)", ""]
        if pm:
            lines += ["counters of the xview_score_kernel dispatches (rocprofv3 --pmc, summed over the device):", ""] + [f"- {c}: {pm[c]:.4g}" for c in COUNTERS if c in pm]
            wc = pm.get("SQ_WAVE_CYCLES")
            if wc:
                lines.append("- of the wave cycles (summed over waves): " +
                             ", ".join(f"{c} {100 * pm[c] / wc:.0f} %" for c in ("SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_LDS_BANK_CONFLICT", "SQ_WAIT_INST_ANY") if c in pm))
            if score_ms and "SQ_ACTIVE_INST_VALU" in pm:
                rate = 4 * pm["SQ_ACTIVE_INST_VALU"] / (4 * MI355X_CUS) / (score_ms * 1e-3) / 1e9
                lines.append(f"- vector-ALU issue cycles per SIMD over the traced kernel time: {rate:.2f} G cycles/s against a clock of at most {MI355X_MAX_GHZ} GHz")
            lines.append("")
        else:
            lines += ["- no counters (rocprofv3 is not installed, gave no rows for the kernel, or a run failed)", ""]
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
