"""Cost of mvhdp_topic_gram at C4 on the state after the benchmark's window: the random start of bench.py, 25 deferred sweeps, then the
calls, each beside the host route it replaces.  Writes a markdown report (default profiles/topic_gram.md).

  timeout -k 10 1100 python tools/topic_gram_timing.py [--workload C4] [--docs D] [--sweeps 25] [--out profiles/topic_gram.md] [--no-profile]

  - ENTITIES over every entity, identity with the counts at threshold 0.03, and sqrt
  - WORDS over every view, identity and sqrt
Wall times are host clocks around the synchronous call: three calls, the median of the last two; stats.kernel_ms is the stream's own time.
The host routes, in full, on at most 16 threads: for ENTITIES theta through doc_topic_proportions in chunks of 50 000 entities and numpy's
dgemm chunk^T . chunk per chunk (plus the sgemm of the 0/1 matrix for the counts); for WORDS get_counts, phi in numpy and one dgemm.
The kernels' own times come from a child run under `rocprofv3 --kernel-trace --stats` on a 200 000-entity model of the same shape running
the ENTITIES call once; it is started only after the wall times were taken without an error, runs under its own time limit in a process
group of its own, and when it fails or runs into the limit the group is killed and nothing more is started on the GPU."""
import argparse
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "16")                               # the host baselines: at most 16 threads
if int(os.environ["OMP_NUM_THREADS"]) > 16:
    os.environ["OMP_NUM_THREADS"] = "16"

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import SEED, ChildFailed, profiled, resource_lines, timed, trained_sampler  # noqa: E402

PARENT_SCORE_RATE = 21.0                                                     # T fp64 FMA/s of xview_score_kernel in profiles/xview_entities.md
KERNELS = r"gram_\w+?_kernel|xview_phi_kernel|doc_topic_prop_kernel"
CHILD_DOCS = 200000
THRESHOLD = 0.03
CHUNK = 50000
TILE_K, TILE_L, BLOCK = 64, 128, 1024


def tiles_launched(K):
    return sum(1 for ti in range((K + TILE_K - 1) // TILE_K) for tj in range((K + TILE_L - 1) // TILE_L) if ti * TILE_K <= min(tj * TILE_L + TILE_L - 1, K - 1))


def host_entities(s, w, D, K, transform, threshold):
    """(ms of theta's round trips, ms of numpy) over all D entities"""
    trip = rest = 0.0
    g, sums = np.zeros((K, K)), np.zeros(K)
    co = np.zeros((K, K), dtype=np.float32)
    for a in range(0, D, CHUNK):
        t0 = time.perf_counter()
        th = s.doc_topic_proportions(w, a, min(a + CHUNK, D))
        t1 = time.perf_counter()
        if threshold is not None:
            ab = (th > threshold).astype(np.float32)
            co += ab.T @ ab
        y = np.sqrt(th) if transform == "sqrt" else th
        g += y.T @ y
        sums += y.sum(0)
        t2 = time.perf_counter()
        trip += (t1 - t0) * 1e3
        rest += (t2 - t1) * 1e3
    return trip, rest, g


def host_words(s, hy, m, transform):
    t0 = time.perf_counter()
    nwk, nk = s.get_counts(m)
    t1 = time.perf_counter()
    phi = (nwk + hy.beta[m]) / (nk + hy.beta_sum[m])
    if hy.inactive is not None:
        phi[:, hy.inactive != 0] = 0.0
    y = np.sqrt(phi) if transform == "sqrt" else phi
    g = y.T @ y
    y.sum(0)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C4")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--sweeps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topic_gram.md"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help="(internal) one ENTITIES call without counts, for the profiler")
    args = ap.parse_args()
    if args.child:
        s = trained_sampler(args.workload, CHILD_DOCS, 2)[0]
        s.topic_gram("entities", view_weights=np.ones(s.M))
        s.close()
        return
    s, hy, corpus, D, _ = trained_sampler(args.workload, args.docs, args.sweeps)
    print(f"{args.sweeps} sweeps done", file=sys.stderr, flush=True)
    K, V, M = s.K, s.V, s.M
    w = np.ones(M)
    tiles = tiles_launched(K)
    lines = ["# mvhdp_topic_gram: timings", "",
             f"Written by tools/topic_gram_timing.py.  Workload {args.workload}" + (f" cut to {args.docs} entities" if args.docs else "") +
             f": K = {K}, V = {V}, {D} entities; the random start of bench.py, then {args.sweeps} deferred sweeps (seed {SEED}).",
             "Wall times: host clock around the synchronous call, the median of 2 calls after 1; kernel_ms: the stream's time from the first kernel to the last.  "
             f"Host routes in full on OMP_NUM_THREADS = {os.environ['OMP_NUM_THREADS']}: theta through doc_topic_proportions in chunks of {CHUNK} entities plus numpy's "
             "dgemm per chunk (and an sgemm of the 0/1 matrix for the counts); get_counts plus phi and one dgemm in numpy.",
             f"FMA counted as rows x K (K + 1) / 2, the cells the contract defines; the kernel executes rows x {tiles} tiles x {TILE_K} x {TILE_L} "
             f"= {tiles * TILE_K * TILE_L / (K * (K + 1) / 2):.2f} times that at K = {K} (tile padding and the cells below the diagonal inside the tiles that straddle it).", ""]
    slower = []

    def report(name, f, base, rows):
        first, med, r = timed(f)
        trip, rest, g = base
        near = bool(np.allclose(r.gram, g, rtol=1e-9, atol=1e-300))
        lines.append(f"- {name}: {med:.1f} ms a call (first call {first:.1f} ms, kernel_ms {r.stats.kernel_ms:.1f}, {r.stats.passes} pass(es) of {r.stats.blocks} blocks) = "
                     f"{rows * K * (K + 1) / 2 / med / 1e9:.2f} T fp64 FMA/s over the whole call; host route: {trip:.0f} ms for the round trip + {rest:.0f} ms of numpy = "
                     f"{(trip + rest) / med:.1f} x the call; numpy's sums agree to 1e-9: {near}")
        print(lines[-1], file=sys.stderr, flush=True)
        if med >= trip + rest:
            slower.append(name)
        return r

    report(f"ENTITIES, identity, counts at threshold {THRESHOLD}, {D} entities", lambda: s.topic_gram("entities", view_weights=w, threshold=THRESHOLD),
           host_entities(s, w, D, K, "identity", THRESHOLD), D)
    report(f"ENTITIES, identity, no counts, {D} entities", lambda: s.topic_gram("entities", view_weights=w), host_entities(s, w, D, K, "identity", None), D)
    report(f"ENTITIES, sqrt, no counts, {D} entities", lambda: s.topic_gram("entities", view_weights=w, transform="sqrt"), host_entities(s, w, D, K, "sqrt", None), D)
    for m in range(M):
        for transform in ("identity", "sqrt"):
            report(f"WORDS, view {m} ({V[m]} types), {transform}", lambda: s.topic_gram("words", m=m, transform=transform), host_words(s, hy, m, transform), V[m])
    s.close()
    lines += ["", "Slower than its host route: " + (", ".join(slower) if slower else "none"), ""]
    lines += ["## the kernels as compiled", ""] + [f"- {l}" for l in resource_lines("mvhdp_gram.hip", r"gram_\w+?_kernel")] + [""]
    if not args.no_profile:
        lines += [f"## the kernels of one ENTITIES call (identity, no counts) on {CHILD_DOCS} entities (a child run of its own, a model trained for 2 sweeps)", ""]
        ks = None
        try:
            print("wall times taken; the kernel trace", file=sys.stderr, flush=True)
            ks = profiled(__file__, ["--workload", args.workload], KERNELS, limit=400)
        except ChildFailed as e:
            lines += [f"- {e}; no further run was started", ""]
        if ks:
            total = sum(ms for _, ms in ks.values())
            for name, (calls, ms) in sorted(ks.items(), key=lambda e: -e[1][1]):
                lines.append(f"- {name}: {ms:.2f} ms over {calls} launch(es), {100 * ms / total:.0f} % of the call's kernel time")
            gram_ms = ks.get("gram_block_kernel", (0, None))[1]
            if gram_ms:
                blocks = (CHILD_DOCS + BLOCK - 1) // BLOCK
                done = CHILD_DOCS * tiles * TILE_K * TILE_L
                useful = CHILD_DOCS * K * (K + 1) // 2
                lines.append(f"- gram_block_kernel: {blocks} blocks x {tiles} tiles; {done} fp64 FMA executed in {gram_ms:.2f} ms = {done / gram_ms / 1e9:.2f} T FMA/s "
                             f"({useful / gram_ms / 1e9:.2f} T/s counted on the cells with k <= l); xview_score_kernel, the same inner loop, in profiles/xview_entities.md: "
                             f"{PARENT_SCORE_RATE} T FMA/s")
            lines.append("")
        else:
            lines += ["- no kernel trace (rocprofv3 is not installed, gave no kernel rows, or the run failed)", ""]
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
