"""Cost of mvhdp_predict_entities / mvhdp_rank_entities at C4 on the state after the benchmark's window: the random start of bench.py, 25
deferred sweeps, then three calls, each beside the path a user has without them.  Writes a markdown report (default
profiles/xview_entities.md).

  python tools/xview_entities_timing.py [--workload C4] [--docs D] [--sweeps 25] [--out profiles/xview_entities.md] [--no-profile]

  (a) predict_entities(m = 1, n = 20): the 20 top entities among all for every type of view 1 (one-item queries)
  (b) predict_entities(m = 0, n = 20): 4096 three-word queries of view 0
  (c) rank_entities(m = 1): 10^5 held-back (item, entity) pairs, the item a type the entity holds in view 1
Wall times are host clocks around the synchronous call: three calls, the median of the last two; stats.kernel_ms is the stream's own
time.  The baseline is theta fetched with doc_topic_proportions, then numpy's dgemm psi . theta^T and argpartition (or a comparison
count per pair) on the host's threads, on a slice of the entities (--baseline-entities), scaled to the entity count by the ratio -- it
is linear in it.  The kernels' own times come from a child run under `rocprofv3 --kernel-trace --stats` on a 50 000-entity model of the
same shape running case (a).  A child that fails or runs into its time limit ends the profiling: its process group is killed and
nothing more is started on the GPU."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import SEED, ChildFailed, profiled, resource_lines, timed, trained_sampler, weights_without  # noqa: E402

PARENT_SCORE_RATE = 20.9                                                     # T fp64 FMA/s of xview_score_kernel in profiles/xview.md
KERNELS = r"xe_\w+|xview_score_kernel|doc_topic_prop_kernel"
COMPILED = r"xe_\w+?_kernel|xview_score_kernel|xview_phi_kernel"
CHILD_DOCS, N_TOP = 50000, 20                                               # tools/xview_timing.py's


def three_word_queries(V, nq, seed=1):
    rng = np.random.default_rng(seed)
    return [[int(x) for x in rng.integers(0, V, 3)] for _ in range(nq)]


def held_pairs(corpus, m, D, n, seed=2):
    """n (item, entity) pairs: entities that hold view m, the item the first type of the span"""
    off, tok = corpus.doc_off[m], corpus.tokens[m]
    has = np.flatnonzero(off[1:D + 1] > off[:D])
    ent = np.random.default_rng(seed).choice(has, size=min(n, len(has)), replace=False).astype(np.int64)
    return tok[off[ent]].astype(np.int64), ent


def host_path(s, hy, m, w, n_ent, items, pairs=None):
    """the path without the calls, on entities [0, n_ent): (ms for theta's round trip, ms for the rest)"""
    t0 = time.perf_counter()
    theta = s.doc_topic_proportions(w, 0, n_ent)
    t1 = time.perf_counter()
    nwk, nk = s.get_counts(m)
    phi = (nwk + hy.beta[m]) / (nk + hy.beta_sum[m])
    if hy.inactive is not None:
        phi[:, hy.inactive != 0] = 0.0
    psi = np.stack([phi[q].sum(0) for q in items]) if isinstance(items, list) else phi[items]
    S = psi @ theta.T
    if pairs is None:
        top = np.argpartition(-S, N_TOP - 1, axis=1)[:, :N_TOP]
        order = np.argsort(-np.take_along_axis(S, top, 1), axis=1, kind="stable")
        np.take_along_axis(top, order, 1)
    else:
        q, e = pairs
        keep = e < n_ent
        (S[q[keep]] > S[q[keep], e[keep]][:, None]).sum(1)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def pick_variant(name, mangled):
    return name + ("<LDS>" if "ILb1E" in mangled else "<memory>" if "ILb0E" in mangled else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C4")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--sweeps", type=int, default=25)
    ap.add_argument("--baseline-entities", type=int, default=20000)
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xview_entities.md"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help="(internal) one predict_entities call of case (a), for the profiler")
    args = ap.parse_args()
    if args.child:
        s = trained_sampler(args.workload, CHILD_DOCS, 2)[0]
        m1 = 1 if s.M > 1 else 0
        s.predict_entities(m1, weights_without(s.M, m1), N_TOP, items=np.arange(s.V[m1], dtype=np.int32))
        s.close()
        return
    s, hy, corpus, D, _ = trained_sampler(args.workload, args.docs, args.sweeps)
    print(f"{args.sweeps} sweeps done", file=sys.stderr, flush=True)
    K, V, M = s.K, s.V, s.M
    m1 = 1 if M > 1 else 0
    nb = min(args.baseline_entities, D)
    lines = ["# mvhdp_predict_entities / mvhdp_rank_entities: timings", "",
             f"Written by tools/xview_entities_timing.py.  Workload {args.workload}" + (f" cut to {args.docs} entities" if args.docs else "") +
             f": K = {K}, V = {V}, {D} entities; the random start of bench.py, then {args.sweeps} deferred sweeps (seed {SEED}).",
             "Wall times: host clock around the synchronous call, the median of 2 calls after 1; kernel_ms: the stream's time from the first kernel to the last.  "
             f"Baseline: theta through doc_topic_proportions, then numpy (dgemm, argpartition / comparison counts) on the host's threads "
             f"(OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}), measured on the first {nb} entities and scaled by the entity count.", ""]

    def report(name, f, base, work, kernel_ms=None):
        first, med, r = timed(f)
        th_ms, rest_ms = base
        scale = D / nb
        kms = kernel_ms(r) if kernel_ms else None
        lines.append(f"- {name}: {med:.1f} ms a call (first call {first:.1f} ms" + (f", kernel_ms {kms:.1f}" if kms is not None else "") +
                     f") = {work / med / 1e9:.2f} T fp64 FMA/s over the whole call; host path: {th_ms * scale:.0f} ms for theta's round trip + "
                     f"{rest_ms * scale:.0f} ms of numpy = {(th_ms + rest_ms) * scale / med:.1f} x the call (measured on {nb} entities: {th_ms:.0f} + {rest_ms:.0f} ms)")
        print(lines[-1], file=sys.stderr, flush=True)
        return r

    w1, w0 = weights_without(M, m1), weights_without(M, 0)
    all_types = np.arange(V[m1], dtype=np.int32)
    report(f"(a) predict_entities(m = {m1}, n = {N_TOP}), every type of view {m1} ({V[m1]} one-item queries), {D} candidates",
           lambda: s.predict_entities(m1, w1, N_TOP, items=all_types), host_path(s, hy, m1, w1, nb, all_types), V[m1] * D * K, lambda r: r.stats.kernel_ms)
    q3 = three_word_queries(V[0], 4096)
    report(f"(b) predict_entities(m = 0, n = {N_TOP}), 4096 three-word queries, {D} candidates",
           lambda: s.predict_entities(0, w0, N_TOP, items=q3), host_path(s, hy, 0, w0, nb, q3), 4096 * D * K, lambda r: r.stats.kernel_ms)
    pq, pe = held_pairs(corpus, m1, D, args.pairs)
    nqp = len(np.unique(pq))
    r = report(f"(c) rank_entities(m = {m1}), {len(pq)} held-back (item, entity) pairs over {nqp} distinct items, {D} candidates",
               lambda: s.rank_entities(m1, w1, pq, pe, items=all_types), host_path(s, hy, m1, w1, nb, all_types, (pq, pe)), nqp * D * K)
    lines += [f"- those pairs: recall@{N_TOP} {r.recall_at(N_TOP):.4f}, MRR {r.mrr():.6f} (the entity itself is excluded for its item and still ranked)", ""]
    s.close()
    lines += ["## the kernels as compiled", ""] + [f"- {l}" for l in resource_lines("mvhdp_xview_entities.hip", COMPILED, pick_variant)] + [""]
    if not args.no_profile:
        lines += [f"## the kernels of one call of case (a) on {CHILD_DOCS} entities (a child run of its own, a model trained for 2 sweeps)", ""]
        ks = None
        try:
            print("wall times taken; the kernel trace", file=sys.stderr, flush=True)
            ks = profiled(__file__, ["--workload", args.workload], KERNELS)
        except ChildFailed as e:
            lines += [f"- {e}; no further run was started", ""]
        if ks:
            total = sum(ms for _, ms in ks.values())
            for name, (calls, ms) in sorted(ks.items(), key=lambda e: -e[1][1]):
                lines.append(f"- {name}: {ms:.2f} ms over {calls} launch(es), {100 * ms / total:.0f} % of the call's kernel time")
            score_ms = ks.get("xview_score_kernel", (0, None))[1]
            if score_ms:
                fma = V[m1] * CHILD_DOCS * K
                lines.append(f"- xview_score_kernel with the roles swapped: nq x D x K = {fma} fp64 FMA in {score_ms:.2f} ms = {fma / score_ms / 1e9:.2f} T FMA/s; "
                             f"the same kernel in profiles/xview.md: {PARENT_SCORE_RATE} T FMA/s")
            lines.append("")
        else:
            lines += ["- no kernel trace (rocprofv3 is not installed, gave no kernel rows, or the run failed)", ""]
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
