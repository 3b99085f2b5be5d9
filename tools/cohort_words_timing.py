"""Cost of mvhdp_cohort_top_words at C4 on the state after the benchmark's window: the random start of bench.py, 25 deferred sweeps, then
the calls, each beside the host route it replaces.  Writes a markdown report (default profiles/cohort_words.md).

  timeout -k 10 1100 python tools/cohort_words_timing.py [--workload C4] [--docs D] [--sweeps 25] [--out profiles/cohort_words.md] [--no-profile]

  (i)   50 cohorts that partition the entities (entity d in cohort d mod 50 -- "years"), views 0 and 1, n = 20, both orders
  (ii)  1000 cohorts of 1000 random entities each, view 0, by share with min_count 2
  (iii) case (i) trends-only
Wall times are host clocks around the synchronous call: three calls, the median of the last two; stats.kernel_ms is the stream's own time.
The host route, in full, on at most 16 threads: mvhdp_get_assignments of the view, then per cohort np.bincount of (z * V + type) over the
cohort's tokens (16 threads over the cohorts) and np.argpartition of every topic's column for the 20 largest counts; for the trends-only
case the bincount of z alone.
The split between the token pass, the clears and the selection comes from a child run under `rocprofv3 --kernel-trace --stats` that
makes the by-count call of case (i) on view 0 once on a 200 000-entity model of the same shape (the tables, and so the clears and the
selection, are those of the full model; the token pass is a fifth); it is started only after the wall times were taken without an error, runs under its
own time limit in a process group of its own, and when it fails or runs into the limit the group is killed and nothing more is started
on the GPU."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

os.environ.setdefault("OMP_NUM_THREADS", "16")                               # the host baselines: at most 16 threads
if int(os.environ["OMP_NUM_THREADS"]) > 16:
    os.environ["OMP_NUM_THREADS"] = "16"

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import SEED, ChildFailed, profiled, timed, trained_sampler  # noqa: E402

FABRIC_PEAK_TBS = 8.0
KERNELS = r"cohort_\w+?_kernel|fillBuffer\w*"
N_TOP = 20
THREADS = 16
CHILD_DOCS = 200000


def partition(D, G=50):
    return [np.arange(g, D, G, dtype=np.int64) for g in range(G)]


def random_cohorts(D, G=1000, size=1000):
    rng = np.random.default_rng(SEED)
    return [rng.integers(0, D, min(size, D)).astype(np.int64) for _ in range(G)]


def csr(cohorts):
    moff = np.zeros(len(cohorts) + 1, dtype=np.int64)
    moff[1:] = np.cumsum([len(c) for c in cohorts])
    return moff, np.concatenate(cohorts)


def host_route(s, corpus, m, cohorts, trends_only):
    """(ms of the assignments' trip, ms of numpy on THREADS threads)"""
    K, V = s.K, s.V[m]
    off, tok = corpus.doc_off[m], corpus.tokens[m]
    t0 = time.perf_counter()
    z = s.get_assignments(m)
    t1 = time.perf_counter()

    def one(members):
        b, e = off[members], off[members + 1]
        n = e - b
        idx = np.repeat(b - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(int(n.sum()))
        zz = z[idx]
        if trends_only:
            return np.bincount(zz, minlength=K)
        c = np.bincount(zz.astype(np.int64) * V + tok[idx], minlength=K * V).reshape(K, V)
        top = np.argpartition(-c, min(N_TOP, V) - 1, axis=1)[:, :N_TOP]
        return np.take_along_axis(c, top, 1)

    with ThreadPoolExecutor(THREADS) as ex:
        list(ex.map(one, cohorts))
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C4")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--sweeps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cohort_words.md"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help="(internal) the by-count call of case (i) on view 0, once, for the profiler")
    args = ap.parse_args()
    if args.child:
        s, _, _, D, _ = trained_sampler(args.workload, min(args.docs or CHILD_DOCS, CHILD_DOCS), 2)
        s.cohort_top_words(0, csr(partition(D)), n=N_TOP)
        s.close()
        return
    s, hy, corpus, D, _ = trained_sampler(args.workload, args.docs, args.sweeps)
    print(f"{args.sweeps} sweeps done", file=sys.stderr, flush=True)
    K, V = s.K, s.V
    lines = ["# mvhdp_cohort_top_words: timings", "",
             f"Written by tools/cohort_words_timing.py.  Workload {args.workload}" + (f" cut to {args.docs} entities" if args.docs else "") +
             f": K = {K}, V = {V}, {D} entities, {[int(corpus.doc_off[m][-1]) for m in range(len(V))]} tokens per view; the random start of bench.py, then "
             f"{args.sweeps} deferred sweeps (seed {SEED}).",
             "Wall times: host clock around the synchronous call, the median of 2 calls after 1; kernel_ms: the stream's time from the first kernel to the last.  "
             f"Host route in full on {THREADS} threads: get_assignments of the view, then per cohort a bincount of (z, type) over its tokens and an argpartition per topic "
             "(trends-only: a bincount of z).", ""]
    slower = []

    def report(name, m, cohorts, host_cohorts, **kw):
        first, med, r = timed(lambda: s.cohort_top_words(m, cohorts, n=N_TOP, **kw))
        trip, rest = host_route(s, corpus, m, host_cohorts, kw.get("trends_only", False))
        st = r.stats
        line = (f"- {name}: {med:.1f} ms a call (first call {first:.1f} ms, kernel_ms {st.kernel_ms:.1f}, {st.passes} pass(es) of {st.cohorts_per_pass} cohorts, "
                f"{st.listings} listings, {st.tokens} tokens counted); host route: {trip:.0f} ms for the assignments' trip + {rest:.0f} ms of numpy = {(trip + rest) / med:.1f} x the call")
        if not kw.get("trends_only", False):
            moved = 2.0 * len(host_cohorts) * K * V[m] * 4                   # one clear and one scan of every cohort's table
            line += f"; the tables' clear and scan move {moved / 1e9:.2f} GB, {moved / (st.kernel_ms * 1e-3) / 1e12:.2f} TB/s over the whole of kernel_ms"
        lines.append(line)
        print(line, file=sys.stderr, flush=True)
        if med >= trip + rest:
            slower.append(name)

    years = partition(D)
    years_csr = csr(years)
    for m in (0, 1):
        for order in ("count", "share"):
            report(f"(i) 50 cohorts that partition the {D} entities, view {m} ({V[m]} types), n = {N_TOP}, by {order}", m, years_csr, years, order=order)
    rnd = random_cohorts(D)
    report(f"(ii) {len(rnd)} cohorts of {len(rnd[0])} random entities, view 0, n = {N_TOP}, by share, min_count 2", 0, csr(rnd), rnd, order="share", min_count=2)
    for m in (0, 1):
        report(f"(iii) case (i) trends-only, view {m}", m, years_csr, years, trends_only=True)
    s.close()
    lines += ["", "Slower than its host route: " + (", ".join(slower) if slower else "none"), ""]
    if not args.no_profile:
        lines += [f"## the kernels of the by-count call of case (i) on view 0 over {min(D, CHILD_DOCS)} entities (a child run of its own, a model trained for 2 sweeps)", ""]
        ks = None
        try:
            print("wall times taken; the kernel trace", file=sys.stderr, flush=True)
            ks = profiled(__file__, ["--workload", args.workload] + (["--docs", str(args.docs)] if args.docs else []), KERNELS, limit=400)
        except ChildFailed as e:
            lines += [f"- {e}; no further run was started", ""]
        if ks:
            total = sum(ms for _, ms in ks.values())
            for name, (calls, ms) in sorted(ks.items(), key=lambda e: -e[1][1]):
                lines.append(f"- {name}: {ms:.2f} ms over {calls} launch(es), {100 * ms / total:.0f} % of the listed kernels' time")
            table = 50 * K * V[0] * 4
            clear = sum(ms for name, (_, ms) in ks.items() if name.startswith("fillBuffer"))
            scan = sum(ms for name, (_, ms) in ks.items() if "select" in name)
            if clear > 0 and scan > 0:
                lines.append(f"- the clears write {table / 1e9:.2f} GB (timed with every other fill of the child run, its training sweeps included) in {clear:.2f} ms = {table / (clear * 1e-3) / 1e12:.2f} TB/s, the selection "
                             f"reads them in {scan:.2f} ms = {table / (scan * 1e-3) / 1e12:.2f} TB/s; together {2 * table / ((clear + scan) * 1e-3) / 1e12:.2f} TB/s "
                             f"= {100 * 2 * table / ((clear + scan) * 1e-3) / 1e12 / FABRIC_PEAK_TBS:.0f} % of the {FABRIC_PEAK_TBS:.0f} TB/s fabric peak")
            lines.append("")
        else:
            lines += ["- no kernel trace (rocprofv3 is not installed, gave no kernel rows, or the run failed)", ""]
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
