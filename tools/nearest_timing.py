"""Cost of mvhdp_nearest_entities / mvhdp_topic_top_entities at C4 on the state after the benchmark's window: the random start of
bench.py, 25 deferred sweeps, then the calls, each beside the path a user has without them.  Writes a markdown report (default
profiles/nearest.md).

  python tools/nearest_timing.py [--workload C4] [--docs D] [--sweeps 25] [--out profiles/nearest.md] [--no-profile]

  - nearest_entities, 65 536 handle queries (entities [0, 65536)) against every entity, n = 20
  - nearest_entities, 1024 host rows (the proportions of the last 1024 entities, downloaded) against every entity, n = 20
  - topic_top_entities, n = 20, every entity
Wall times are host clocks around the synchronous call: one warm-up call, then --repeats calls; the median, the smallest and the largest
are reported.  Baselines: theta fetched with doc_topic_proportions (timed on its own), then numpy on the host's threads -- normalised rows,
dgemm against a subset of the queries (--baseline-queries) and argpartition per row, scaled by the query count (it is linear in it); for
topic_top_entities the same round trip plus numpy.argpartition per topic.  The tile kernel's own time comes from a child run under
`rocprofv3 --kernel-trace --stats` on a smaller call (--child-queries handle queries); a child that fails or runs into its time limit
ends the profiling: its process group is killed and nothing more is started on the GPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import SEED, ChildFailed, profiled, trained_sampler  # noqa: E402

N_TOP = 20
PEAK_TF, UNTUNED_TF = 155.0, 122.0                                           # fp32 MFMA: measured peak, and an untuned 4096^3 tile kernel on the same instruction
KERNELS = r"near_\w+|topk_\w+|sim_prepare_kernel|sim_normalise_kernel|doc_topic_prop_kernel"


def timed(f, repeats):
    f()                                                                      # warm-up: allocations, the carry-over maps
    out, r = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = f()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out), r


def host_nearest(theta, q, n):
    """the path without the call, on the downloaded proportions: cosine by dgemm, the first n per row"""
    t0 = time.perf_counter()
    xn = theta / np.sqrt((theta * theta).sum(1))[:, None]
    t1 = time.perf_counter()
    qn = q / np.sqrt((q * q).sum(1))[:, None]
    S = qn @ xn.T
    top = np.argpartition(-S, n - 1, axis=1)[:, :n]
    order = np.argsort(-np.take_along_axis(S, top, 1), axis=1, kind="stable")
    np.take_along_axis(top, order, 1)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def host_topic_top(theta, n):
    t0 = time.perf_counter()
    top = np.argpartition(-theta, n - 1, axis=0)[:n]
    order = np.argsort(-np.take_along_axis(theta, top, 0), axis=0, kind="stable")
    np.take_along_axis(top, order, 0)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C4")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--sweeps", type=int, default=25)
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--host-queries", type=int, default=1024)
    ap.add_argument("--baseline-queries", type=int, default=256)
    ap.add_argument("--child-queries", type=int, default=8192)
    ap.add_argument("--child-docs", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest.md"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help="(internal) one nearest_entities call, for the profiler")
    args = ap.parse_args()
    if args.child:
        s, _, _, D, _ = trained_sampler(args.workload, args.child_docs, 2)
        s.nearest_entities(np.ones(s.M), N_TOP, q0=0, q1=min(args.child_queries, D))
        s.close()
        return
    s, _, _, D, _ = trained_sampler(args.workload, args.docs, args.sweeps)
    print(f"{args.sweeps} sweeps done", file=sys.stderr, flush=True)
    K, M = s.K, s.M
    w = np.ones(M)
    nq, nh, nb = min(args.queries, D), min(args.host_queries, D), min(args.baseline_queries, D)
    lines = ["# mvhdp_nearest_entities / mvhdp_topic_top_entities: timings", "",
             f"Written by tools/nearest_timing.py.  Workload {args.workload}" + (f" cut to {args.docs} entities" if args.docs else "") +
             f": K = {K}, V = {s.V}, {D} entities; the random start of bench.py, then {args.sweeps} deferred sweeps (seed {SEED}); view weights 1.",
             f"Wall times: host clock around the synchronous call, one warm-up call, then {args.repeats}: median (smallest .. largest).  Baseline: theta "
             f"through doc_topic_proportions, then numpy on the host's threads (OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')}).", ""]

    def say(text):
        lines.append(text)
        print(text, file=sys.stderr, flush=True)

    t0 = time.perf_counter()
    theta = s.doc_topic_proportions(w)
    trip = (time.perf_counter() - t0) * 1e3
    say(f"- doc_topic_proportions round trip, {D} entities ({theta.nbytes / 1e9:.2f} GB to the host): {trip:.0f} ms")
    norm_ms, rest_ms = host_nearest(theta, theta[:nb], N_TOP)
    say(f"- host path for {nb} queries: {norm_ms:.0f} ms to normalise the rows + {rest_ms:.0f} ms of dgemm and argpartition = {rest_ms / nb:.2f} ms a query")

    med, lo, hi, r = timed(lambda: s.nearest_entities(w, N_TOP, q0=0, q1=nq), args.repeats)
    st = r.stats
    flop = 2.0 * st.cells_screened * ((K + 31) // 32 * 32)
    say(f"- nearest_entities, {nq} handle queries x {D} candidates, n = {N_TOP}: {med:.0f} ms ({lo:.0f} .. {hi:.0f}) = {1e3 * med / nq:.1f} us a query; "
        f"{st.blocks} blocks, {st.cells_screened} cells screened, {st.candidates} candidates = {st.candidates / nq:.2f} a query, {st.exact_only_rows} rows not screened, "
        f"regrown {st.regrown}; the screen's {flop / 1e12:.1f} TFLOP over the WHOLE call: {flop / med / 1e9:.1f} TFLOP/s")
    say(f"- extrapolated, not measured: the self-neighbour graph of all {D} entities at that rate per query: {med * D / nq / 1e3:.1f} s")
    base = trip + norm_ms + rest_ms * nq / nb
    say(f"- the same by the host path: {trip:.0f} + {norm_ms:.0f} + {rest_ms * nq / nb:.0f} ms (scaled from {nb} queries) = {base / med:.1f} x the call")
    qh = np.ascontiguousarray(theta[D - nh:])
    med, lo, hi, r = timed(lambda: s.nearest_entities(w, N_TOP, queries=qh), args.repeats)
    say(f"- nearest_entities, {nh} host rows x {D} candidates, n = {N_TOP}: {med:.0f} ms ({lo:.0f} .. {hi:.0f}) = {1e3 * med / nh:.1f} us a query; "
        f"{r.stats.candidates / nh:.2f} candidates a query; host path {trip:.0f} + {norm_ms:.0f} + {rest_ms * nh / nb:.0f} ms = {(trip + norm_ms + rest_ms * nh / nb) / med:.1f} x the call")
    med, lo, hi, r = timed(lambda: s.topic_top_entities(w, N_TOP), args.repeats)
    top_ms = host_topic_top(theta, N_TOP)
    say(f"- topic_top_entities, n = {N_TOP}, {D} entities, K = {K}: {med:.0f} ms ({lo:.0f} .. {hi:.0f}); host path {trip:.0f} ms round trip + {top_ms:.0f} ms of "
        f"argpartition per topic = {(trip + top_ms) / med:.1f} x the call")
    lines.append("")
    s.close()
    del theta
    if not args.no_profile:
        cq, cd = args.child_queries, args.child_docs
        lines += [f"## the kernels of one nearest_entities call, {cq} handle queries x {cd} candidates (a child run of its own, a model trained for 2 sweeps)", ""]
        try:
            print("wall times taken; the kernel trace", file=sys.stderr, flush=True)
            ks = profiled(__file__, ["--workload", args.workload, "--child-queries", str(cq), "--child-docs", str(cd)], KERNELS, limit=420)
        except ChildFailed as e:
            ks = None
            lines += [f"- {e}; no further run was started", ""]
        if ks:
            total = sum(ms for _, ms in ks.values())
            for name, (calls, ms) in sorted(ks.items(), key=lambda e: -e[1][1]):
                lines.append(f"- {name}: {ms:.2f} ms over {calls} launch(es), {100 * ms / total:.0f} % of the call's kernel time")
            if "near_screen_kernel" in ks:
                from mvtopicmodel_amd.native import nearest_probe
                ms = ks["near_screen_kernel"][1]
                useful = 2.0 * cq * cd * K
                padded = 2.0 * nearest_probe(cq, cd, K).cells_screened * ((K + 31) // 32 * 32)
                lines.append(f"- near_screen_kernel: {useful / 1e12:.2f} TFLOP at the useful size ({padded / 1e12:.2f} with tile and k padding) in {ms:.2f} ms = "
                             f"{useful / ms / 1e9:.1f} TFLOP/s ({100 * useful / ms / 1e9 / PEAK_TF:.0f} % of the {PEAK_TF:.0f} TF fp32-MFMA peak of v_mfma_f32_32x32x2_f32, "
                             f"{100 * useful / ms / 1e9 / UNTUNED_TF:.0f} % of the {UNTUNED_TF:.0f} TF an untuned tile kernel reaches at 4096^3)")
            lines.append("")
        else:
            lines += ["- no kernel trace (rocprofv3 is not installed, gave no kernel rows, or the run failed): the tile kernel's own rate is MISSING", ""]
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
