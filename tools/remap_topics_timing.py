"""Cost of mvhdp_remap_topics at C4 on the state after the benchmark's window: the random start of bench.py, 25 deferred sweeps, then the
call with two maps, each beside the host route it replaces.  Writes a markdown report (default profiles/remap_topics.md).

  timeout -k 10 900 python tools/remap_topics_timing.py [--workload C4] [--docs D] [--sweeps 25] [--out profiles/remap_topics.md] [--no-profile]

  (i)  a 20-pair merge map: the 20 most similar topic pairs of mvhdp_topic_gram over the view-0 words (cosine), through surgery.merge_map
  (ii) a full reordering: surgery.order_map of the topics' token counts
Every timed call starts from the same state (the assignments, counts and hyper-parameters after the sweeps, put back through the host
before it).  Wall times are host clocks around the synchronous call: three calls, the median of the last two; stats.kernel_ms is the
stream's own time over both passes.
The host route, in full, through the existing API in the same process: get_assignments of every view, a numpy take through the map,
set_assignments back, build_counts, and set_hyper with alpha and the inactive set folded by numpy.
The bytes: the assignment pass reads 4 bytes a token and writes 16 for every group of four tokens in which one changed (bounded below by 4
bytes per changed token, above by 16); the fold pass reads 4 bytes per count cell of the sumV + M rows and writes the cells that changed
(counted here on the host from the counts before and after).
The split between the two passes comes from a child run under `rocprofv3 --kernel-trace --stats` that makes each call once on a
200 000-entity model of the same shape (the count table, and so the fold pass, is the full model's; the assignment pass is a fifth); it is
started only after the wall times were taken without an error, runs under its own time limit in a process group of its own, and when it
fails or runs into the limit the group is killed and nothing more is started on the GPU."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import SEED, ChildFailed, profiled, trained_sampler  # noqa: E402

from mvtopicmodel_amd import surgery  # noqa: E402
from mvtopicmodel_amd.native import Hyper  # noqa: E402

FABRIC_PEAK_TBS = 8.0
KERNELS = r"remap_\w+?_kernel"
CHILD_DOCS = 200000
PAIRS = 20


def merge_pairs_map(s, weight, pairs=PAIRS):
    """the `pairs` most similar topic pairs by the cosine of their view-0 word columns, merged onto the heavier topic"""
    sim = np.nan_to_num(s.topic_gram("words", m=0).cosine(), nan=-1.0)
    np.fill_diagonal(sim, -1.0)
    upper = np.triu(sim, 1)
    upper[np.tril_indices(s.K)] = -1.0
    cut = np.sort(upper, axis=None)[-pairs - 1] if s.K * (s.K - 1) // 2 > pairs else -1.0
    return surgery.merge_map(np.where(upper > cut, upper, -1.0), cut, weight)


def weights(s):
    return sum(s.get_counts(m)[1].astype(np.int64) for m in range(s.M))


def fold_hyper(hy, alpha, inactive, tm):
    """alpha and the inactive set through the map, by numpy (sums by np.add.at: the host route is not pinned to the call's bits)"""
    K = len(tm)
    out = Hyper(**{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in vars(hy).items()})
    on = tm >= 0
    a = np.zeros_like(alpha)
    a[:, K] = alpha[:, K]
    for m in range(alpha.shape[0]):
        np.add.at(a[m], tm[on], alpha[m, :K][on])
    has = np.zeros(K, dtype=bool)
    has[tm[on]] = True
    act = np.zeros(K, dtype=bool)
    act[tm[on & (inactive == 0)]] = True
    out.alpha = a
    out.inactive = np.where(has, ~act, inactive != 0).astype(np.uint8)
    return out


def restore(s, hy, z0, alpha0, inactive0):
    for m in range(s.M):
        s.set_assignments(m, z0[m])
    h = Hyper(**vars(hy))
    h.alpha, h.inactive = alpha0, inactive0
    s.set_hyper(h)
    s.build_counts()


def host_route(s, hy, tm):
    """ms of every step of the route through the host"""
    t = [time.perf_counter()]
    z = [s.get_assignments(m) for m in range(s.M)]
    t.append(time.perf_counter())
    z = [np.where(x >= 0, tm[np.maximum(x, 0)], -1).astype(np.int32) for x in z]
    t.append(time.perf_counter())
    for m in range(s.M):
        s.set_assignments(m, z[m])
    t.append(time.perf_counter())
    s.build_counts()
    t.append(time.perf_counter())
    alpha, inactive = s.get_alpha()
    s.set_hyper(fold_hyper(hy, alpha, inactive, tm))
    t.append(time.perf_counter())
    return [(b - a) * 1e3 for a, b in zip(t, t[1:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C4")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--sweeps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remap_topics.md"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help="(internal) each of the two calls once, for the profiler")
    args = ap.parse_args()
    if args.child:
        s = trained_sampler(args.workload, min(args.docs or CHILD_DOCS, CHILD_DOCS), 2)[0]
        w = weights(s)
        s.remap_topics(merge_pairs_map(s, w))
        s.remap_topics(surgery.order_map(weights(s), s.get_alpha()[1]))
        s.close()
        return
    s, hy, corpus, D, _ = trained_sampler(args.workload, args.docs, args.sweeps)
    print(f"{args.sweeps} sweeps done", file=sys.stderr, flush=True)
    K, V, M = s.K, s.V, s.M
    N = [int(corpus.doc_off[m][-1]) for m in range(M)]
    z0 = [s.get_assignments(m) for m in range(M)]
    alpha0, inactive0 = s.get_alpha()
    w = weights(s)
    cells = (sum(V) + M) * K
    lines = ["# mvhdp_remap_topics: timings", "",
             f"Written by tools/remap_topics_timing.py.  Workload {args.workload}" + (f" cut to {args.docs} entities" if args.docs else "") +
             f": K = {K}, V = {V}, {D} entities, {N} tokens per view ({4 * sum(N) / 1e6:.0f} MB of assignments, {4 * cells / 1e6:.0f} MB of counts); the random start of "
             f"bench.py, then {args.sweeps} deferred sweeps (seed {SEED}).",
             "Wall times: host clock around the synchronous call, the median of 2 calls after 1, every call from the same restored state; kernel_ms: the "
             "stream's time over both passes.  Host route in full through the existing API: get_assignments of every view, a numpy take, set_assignments, "
             "build_counts, set_hyper with alpha and the inactive set folded by numpy.", ""]
    slower = []
    cases = [(f"(i) a {PAIRS}-pair merge map (the most similar pairs of topic_gram over the view-0 words)", merge_pairs_map(s, w)),
             ("(ii) a full reordering (order_map of the topics' token counts)", surgery.order_map(w, inactive0))]
    for name, tm in cases:
        before = [np.concatenate([c.ravel() for c in s.get_counts(m)]) for m in range(M)]

        def call():
            restore(s, hy, z0, alpha0, inactive0)
            t0 = time.perf_counter()
            st = s.remap_topics(tm)
            return (time.perf_counter() - t0) * 1e3, st

        runs = [call() for _ in range(3)]
        first, med, st = runs[0][0], float(np.median([r[0] for r in runs[1:]])), runs[-1][1]
        after = [np.concatenate([c.ravel() for c in s.get_counts(m)]) for m in range(M)]
        cells_written = int(sum((a != b).sum() for a, b in zip(before, after)))
        changed = int(st.moved.sum() + st.dropped.sum())
        lo = 4 * sum(N) + 4 * changed + 4 * cells + 4 * cells_written
        hi = lo + 12 * min(changed, sum(N) // 4 + 1)
        restore(s, hy, z0, alpha0, inactive0)
        steps = host_route(s, hy, tm)
        host = sum(steps)
        line = (f"- {name}: {med:.2f} ms a call (first call {first:.2f} ms, kernel_ms {st.kernel_ms:.3f}); {int((tm != np.arange(K)).sum())} of {K} map entries move, "
                f"{int(st.moved.sum())} tokens moved, {int(st.dropped.sum())} dropped, {cells_written} count cells rewritten; both passes move {lo / 1e6:.0f} to {hi / 1e6:.0f} MB, "
                f"{lo / (st.kernel_ms * 1e-3) / 1e12:.2f} to {hi / (st.kernel_ms * 1e-3) / 1e12:.2f} TB/s over kernel_ms = {100 * lo / (st.kernel_ms * 1e-3) / 1e12 / FABRIC_PEAK_TBS:.0f} to "
                f"{100 * hi / (st.kernel_ms * 1e-3) / 1e12 / FABRIC_PEAK_TBS:.0f} % of the {FABRIC_PEAK_TBS:.0f} TB/s fabric peak; host route: "
                f"{steps[0]:.0f} ms get_assignments + {steps[1]:.0f} ms numpy + {steps[2]:.0f} ms set_assignments + {steps[3]:.1f} ms build_counts + {steps[4]:.1f} ms set_hyper = "
                f"{host:.0f} ms = {host / med:.0f} x the call")
        lines.append(line)
        print(line, file=sys.stderr, flush=True)
        if med >= host:
            slower.append(name)
    s.close()
    lines += ["", "Slower than its host route: " + (", ".join(slower) if slower else "none"), ""]
    if not args.no_profile:
        lines += [f"## the kernels of the two calls over {min(D, CHILD_DOCS)} entities (a child run of its own, a model trained for 2 sweeps)", ""]
        ks = None
        try:
            print("wall times taken; the kernel trace", file=sys.stderr, flush=True)
            ks = profiled(__file__, ["--workload", args.workload] + (["--docs", str(args.docs)] if args.docs else []), KERNELS, limit=400)
        except ChildFailed as e:
            lines += [f"- {e}; no further run was started", ""]
        if ks:
            for name, (calls, ms) in sorted(ks.items(), key=lambda e: -e[1][1]):
                lines.append(f"- {name}: {ms:.3f} ms over {calls} launch(es)")
            fold = sum(ms for name, (_, ms) in ks.items() if "fold" in name)
            zk = sum(ms for name, (_, ms) in ks.items() if "remap_z" in name)
            n_child = sum(N) * min(D, CHILD_DOCS) / D
            if fold > 0:
                lines.append(f"- the fold pass reads {2 * 4 * cells / 1e6:.0f} MB over the two calls in {fold:.3f} ms: at least {2 * 4 * cells / (fold * 1e-3) / 1e12:.2f} TB/s "
                             f"= {100 * 2 * 4 * cells / (fold * 1e-3) / 1e12 / FABRIC_PEAK_TBS:.0f} % of the fabric peak")
            if zk > 0:
                lines.append(f"- the assignment pass reads about {2 * 4 * n_child / 1e6:.0f} MB over the two calls in {zk:.3f} ms: at least {2 * 4 * n_child / (zk * 1e-3) / 1e12:.2f} TB/s "
                             f"= {100 * 2 * 4 * n_child / (zk * 1e-3) / 1e12 / FABRIC_PEAK_TBS:.0f} % of the fabric peak")
            lines.append("")
        else:
            lines += ["- no kernel trace (rocprofv3 is not installed, gave no kernel rows, or the run failed)", ""]
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
