"""Cost of mvhdp_split_topic at C4 on the state after the benchmark's window: the random start of bench.py, 25 deferred sweeps, then the
heaviest topic split with 20 iterations, beside the host route it replaces and one deferred sweep.  Writes a markdown report (default
profiles/split_topic.md).

  timeout -k 10 900 python tools/split_topic_timing.py [--workload C4] [--docs D] [--sweeps 25] [--iterations 20] [--out profiles/split_topic.md]
  rocprofv3 --kernel-trace --stats -d DIR -o st --output-format csv -- python tools/split_topic_timing.py --child --docs 200000

A workload without an inactive topic (C4) gets its free index the way a user would make one: the lightest topic is merged into the second
lightest by mvhdp_remap_topics with MVHDP_REMAP_RETIRE.  Every timed call starts from the same state (the assignments, counts and
hyper-parameters put back through the host before it).  Wall times are host clocks around the synchronous call: three calls, the median
of the last two; stats.kernel_ms is the stream's own time over the kernels of the call.
Pass 0 and the iterations: the call with iterations = 0 is the two passes over z (count, then list with the initial sides), the CSR, the
table fill and the last pass; the cost of an iteration is (kernel_ms at `iterations` - kernel_ms at 0) / iterations.
The bytes of pass 0: every view's z is read twice, 8 bytes a token (the lists, the table and the two columns are small beside it), so
bytes / kernel_ms at 0 iterations is a LOWER bound of the scan's bandwidth.  mvhdp_remap_topics with the identity map beside it: its z pass
reads 4 bytes a token and its fold pass 4 bytes a count cell.
The host route, in full, in the same process: get_assignments of every view, the sequential restatement of the contract
(tests/native/split_ref.c, one thread), set_assignments back, build_counts, set_hyper."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import SEED, trained_sampler  # noqa: E402

from mvtopicmodel_amd import surgery  # noqa: E402
from mvtopicmodel_amd.native import Hyper  # noqa: E402
from tests import split_cases, split_ref  # noqa: E402

FABRIC_PEAK_TBS = 8.0
BINS = [1, 2, 4, 8, 16, 64, 1024, 1 << 62]


def weights(s):
    return sum(s.get_counts(m)[1].astype(np.int64) for m in range(s.M))


def with_state(hy, alpha, inactive):
    h = Hyper(**vars(hy))
    h.alpha, h.inactive = alpha, inactive
    return h


def restore(s, hy, z0, alpha0, inactive0):
    for m in range(s.M):
        s.set_assignments(m, z0[m])
    s.set_hyper(with_state(hy, alpha0, inactive0))
    s.build_counts()


def timed_split(s, restore_fn, **kw):
    runs = []
    for _ in range(3):
        restore_fn()
        t0 = time.perf_counter()
        st = s.split_topic(**kw)
        runs.append(((time.perf_counter() - t0) * 1e3, st))
    return runs[0][0], float(np.median([r[0] for r in runs[1:]])), float(np.median([r[1].kernel_ms for r in runs[1:]])), runs[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C4")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--sweeps", type=int, default=25)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_topic.md"))
    ap.add_argument("--child", action="store_true", help="one split after 2 sweeps and nothing else: the run to put under a kernel trace")
    args = ap.parse_args()
    if args.child:
        s = trained_sampler(args.workload, args.docs, 2)[0]
        w = weights(s)
        light = np.argsort(w, kind="stable")[:2]
        tm = surgery.identity_map(s.K)
        tm[light[0]] = light[1]
        s.remap_topics(tm, retire=True)
        st = s.split_topic(int(np.argmax(weights(s))), iterations=args.iterations, seed=SEED)
        print(f"split {int(st.split.sum())} tokens, kernel_ms {st.kernel_ms:.3f}")
        s.close()
        return
    s, hy, corpus, D, _ = trained_sampler(args.workload, args.docs, args.sweeps)
    print(f"{args.sweeps} sweeps done", file=sys.stderr, flush=True)
    K, V, M = s.K, s.V, s.M
    N = [int(corpus.doc_off[m][-1]) for m in range(M)]
    w = weights(s)
    alpha, inactive = s.get_alpha()
    made = ""
    if len(surgery.free_topics(w, inactive, alpha)) == 0:
        light = np.argsort(w, kind="stable")[:2]
        tm = surgery.identity_map(K)
        tm[light[0]] = light[1]
        s.remap_topics(tm, retire=True)
        made = f"  The workload has no inactive topic: topic {int(light[0])} ({int(w[light[0]])} tokens) was merged into topic {int(light[1])} with RETIRE first."
    z0 = [s.get_assignments(m) for m in range(M)]
    alpha0, inactive0 = s.get_alpha()
    w = weights(s)
    source = int(np.argmax(w))
    free = surgery.free_topics(w, inactive0, alpha0)
    back = lambda: restore(s, hy, z0, alpha0, inactive0)
    cells = (sum(V) + M) * K
    lines = ["# mvhdp_split_topic: timings", "",
             f"Written by tools/split_topic_timing.py; every figure below was measured in that one run unless it says otherwise.  Workload {args.workload}" +
             (f" cut to {args.docs} entities" if args.docs else "") +
             f": K = {K}, V = {V}, {D} entities, {N} tokens per view ({4 * sum(N) / 1e6:.0f} MB of assignments, {4 * cells / 1e6:.0f} MB of counts); the random start "
             f"of bench.py, then {args.sweeps} deferred sweeps (seed {SEED}).{made}",
             f"The source is the heaviest topic, {source} ({int(w[source])} tokens = 1/{sum(N) / max(int(w[source]), 1):.0f} of all); the target is the library's pick, {int(free[0])}.", ""]

    # the list lengths: what decides lane-per-entity against wave-per-entity
    per_entity = np.zeros(D, dtype=np.int64)
    for m in range(M):
        c = np.concatenate([[0], np.cumsum(z0[m] == source)])
        per_entity += np.diff(c[corpus.doc_off[m]])
    owners = per_entity[per_entity > 0]
    hist = np.histogram(owners, bins=BINS)[0]
    lines += [f"- entities that own tokens of the set: {len(owners)} of {D}; tokens of the set per owner: mean {owners.mean():.1f}, max {int(owners.max())}; owners by list length "
              + ", ".join(f"[{a}, {b}): {int(h)}" for a, b, h in zip(BINS, BINS[1:-1] + ["inf"], hist)), ""]

    first, med, kms, st = timed_split(s, back, source=source, iterations=args.iterations, seed=SEED)
    first0, med0, kms0, st0 = timed_split(s, back, source=source, iterations=0, seed=SEED)
    per_it = (kms - kms0) / max(args.iterations, 1)
    scan_bytes = 8 * sum(N)
    lines += [f"- the split with {args.iterations} iterations: {med:.2f} ms a call (first call {first:.2f} ms), kernel_ms {kms:.3f}; {int(st.split.sum())} tokens in the set, "
              f"{int(st.moved.sum())} in the target at the end, flips per iteration {st.flips.tolist()}",
              f"- the same with 0 iterations (pass 0, the table, the last pass): {med0:.2f} ms a call (first call {first0:.2f} ms), kernel_ms {kms0:.3f}",
              f"- one iteration (a sampling launch and an apply launch): ({kms:.3f} - {kms0:.3f}) / {args.iterations} = {per_it:.3f} ms = "
              f"{per_it * 1e6 / max(int(st.split.sum()), 1):.2f} ns per token of the set",
              f"- pass 0 reads every z twice, {scan_bytes / 1e6:.0f} MB: at least {scan_bytes / (kms0 * 1e-3) / 1e12:.2f} TB/s over kernel_ms at 0 iterations "
              f"= {100 * scan_bytes / (kms0 * 1e-3) / 1e12 / FABRIC_PEAK_TBS:.0f} % of the {FABRIC_PEAK_TBS:.0f} TB/s fabric peak (a lower bound: the other kernels of the call and a host "
              "round trip for the block counts are inside kernel_ms)"]
    back()
    rs = [s.remap_topics(surgery.identity_map(K)) for _ in range(3)]
    rk = float(np.median([r.kernel_ms for r in rs[1:]]))
    rb = 4 * sum(N) + 4 * cells
    lines += [f"- mvhdp_remap_topics with the identity map on the same state: kernel_ms {rk:.3f} for {rb / 1e6:.0f} MB read (z once, the count rows once) = "
              f"{rb / (rk * 1e-3) / 1e12:.2f} TB/s"]

    # one deferred sweep (the sweep's code is what it was before this call existed)
    back()
    s.sweep(args.sweeps, SEED)
    t0 = time.perf_counter()
    sw = s.sweep(args.sweeps + 1, SEED)
    sweep_ms = (time.perf_counter() - t0) * 1e3
    lines += [f"- one deferred sweep on the same state: {sweep_ms:.1f} ms a call over {int(sw.tokens)} tokens; one iteration of the split is {100 * per_it / sweep_ms:.2f} % of it, "
              f"the whole call with {args.iterations} iterations {100 * med / sweep_ms:.0f} %"]

    # the host route
    back()
    t = [time.perf_counter()]
    z = [s.get_assignments(m) for m in range(M)]
    t.append(time.perf_counter())
    nk = np.stack([s.get_counts(m)[1] for m in range(M)])
    t.append(time.perf_counter())
    ref = split_ref.run(K, V, corpus.doc_off, corpus.tokens, z, with_state(hy, alpha0, inactive0), source, iterations=args.iterations, seed=SEED, nk=nk)
    t.append(time.perf_counter())
    for m in range(M):
        s.set_assignments(m, ref.z[m])
    t.append(time.perf_counter())
    s.build_counts()
    t.append(time.perf_counter())
    s.set_hyper(with_state(hy, ref.alpha, ref.inactive))
    t.append(time.perf_counter())
    steps = [(b - a) * 1e3 for a, b in zip(t, t[1:])]
    same = np.array_equal(ref.flips, st.flips) and np.array_equal(ref.moved, st.moved) and ref.target == st.target
    host = sum(steps)
    lines += [f"- the host route: {steps[0]:.0f} ms get_assignments + {steps[1]:.0f} ms n_k + {steps[2]:.0f} ms the restatement on one thread + {steps[3]:.0f} ms set_assignments + "
              f"{steps[4]:.1f} ms build_counts + {steps[5]:.1f} ms set_hyper = {host:.0f} ms = {host / med:.0f} x the call; its flips per iteration, moved counts and target equal the device's: {same}", ""]
    s.close()

    # the planted case of tests/split_cases.py on the restatement (no device): with and without hints
    lines += ["## the planted case (tests/split_cases.py, the restatement alone, 20 iterations, seed 2)", ""]
    for hinted in (True, False):
        c = split_cases.planted(hinted=hinted)
        r = split_ref.run(c.K, c.V, c.doc_off, c.tokens, c.z, c.hy, c.source, iterations=20, seed=2, type_hint=c.hint)
        p = split_cases.purity(c, r.z, r.target)
        lines.append(f"- {'two anchors hinted per vocabulary' if hinted else 'no hints (the sides may come out swapped: purity p and 1 - p are the same split)'}: "
                     f"purity {p:.4f}, flips {r.flips.tolist()}")
    lines.append("")
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
