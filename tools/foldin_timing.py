"""Cost of mvhdp_fold_in at C4 on the state after the benchmark's window: the random start of bench.py, 25 deferred sweeps, then the
generator's NEXT entities under the training seed (unseen documents of the training topics, all views) folded in with 10 iterations --
65 536 and 10^6 of them -- beside the route the library had before: a second handle of the same shape, the counts copied through the
host, the hyper-parameters, the corpus, inference trees, the tree-sampled start, ten MVHDP_SWEEP_FROZEN sweeps, the proportions.
Appends a markdown section to the report (default profiles/foldin.md, below its hand-written head).

  python tools/foldin_timing.py [--workload C4] [--docs D] [--sweeps 25] [--sizes 65536,1000000] [--out profiles/foldin.md]

Wall times are host clocks around the synchronous call (the method of profiles/heldout.md); kernel_ms is the library's own event pair
around its kernel launches.  Device memory: the drop of the device's free memory (hipMemGetInfo through torch, when it is installed)
while the second handle exists; the fold-in's scratch is bounded by construction (csrc/mvhdp_foldin.hip says by what)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import SEED, timed, trained_sampler  # noqa: E402

ITERATIONS = 10


def free_bytes():
    try:
        import torch
        return int(torch.cuda.mem_get_info()[0])
    except Exception:
        return None


def second_handle_route(s, hy, K, V, off, tok, w):
    """the kit of parts, stage by stage: ({stage: ms}, theta, bytes of device memory the second handle held)"""
    from mvtopicmodel_amd import NativeSampler
    from mvtopicmodel_amd.native import SWEEP_FROZEN
    ms = {}

    def stage(name, t0):
        ms[name] = ms.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
    free0 = free_bytes()
    t0 = time.perf_counter(); s2 = NativeSampler(K, V); stage("create", t0)
    try:
        t0 = time.perf_counter()
        for m in range(len(V)):
            s2.set_corpus(m, off[m], tok[m])                                 # (first: a new corpus forgets the counts)
        stage("set_corpus", t0)
        t0 = time.perf_counter(); s2.set_hyper(hy); stage("set_hyper", t0)
        t0 = time.perf_counter()
        for m in range(len(V)):
            s2.set_counts(m, *s.get_counts(m))
        stage("counts copy (get_counts -> set_counts)", t0)
        t0 = time.perf_counter(); s2.build_inference_trees(); stage("build_inference_trees", t0)
        t0 = time.perf_counter(); s2.init_assignments_from_trees(SEED); stage("init_assignments_from_trees", t0)
        t0 = time.perf_counter()
        for i in range(ITERATIONS):
            s2.sweep(i, SEED, flags=SWEEP_FROZEN)
        stage("%d frozen sweeps" % ITERATIONS, t0)
        t0 = time.perf_counter(); theta = s2.doc_topic_proportions(w); stage("doc_topic_proportions", t0)
        free1 = free_bytes()
    finally:
        s2.close()
    return ms, theta, (free0 - free1) if free0 is not None and free1 is not None else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C4")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--sweeps", type=int, default=25)
    ap.add_argument("--sizes", default="65536,1000000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "foldin.md"))
    args = ap.parse_args()
    from mvtopicmodel_amd import synth
    s, hy, _, D, sweeps = trained_sampler(args.workload, args.docs, args.sweeps)
    sweep_ms, sweep_tokens = [x.total_ms for x in sweeps], sweeps[-1].tokens
    free_bytes()                                                             # (torch's first device query, outside every timed region)
    c = dict(synth.CONFIGS[args.workload])
    K, V, M = c["K"], c["V"], len(c["V"])
    w = np.array([1.0] + [0.5] * (M - 1))
    settled = statistics.median(sweep_ms[5:]) if len(sweep_ms) > 5 else statistics.median(sweep_ms)
    lines = ["", "## Measured: tools/foldin_timing.py", "",
             f"Workload {args.workload}: K = {K}, V = {V}, {D} entities; the random start of bench.py, then {args.sweeps} deferred sweeps "
             f"(seed {SEED}; median of sweeps 5.. {settled:.1f} ms for {sweep_tokens} tokens = {sweep_tokens / settled / 1e6:.2f} G tokens/s).",
             f"Folded in: the generator's next entities under the training seed, all {M} views, {ITERATIONS} iterations, samples = 1, "
             f"view weights {[float(x) for x in w]}.  Wall: host clock around the synchronous call.", ""]
    for n in [int(x) for x in args.sizes.split(",")]:
        nxt = synth.generate(c["K"], c["V"], D + n, c["lam"], c["seed"], power_law_text=c.get("power_law_text", False), doc_lo=D, doc_hi=D + n)
        off, tok = list(nxt.doc_off), list(nxt.tokens)
        ntok = sum(len(t) for t in tok)
        calls = 3 if n <= 100000 else 2
        first, med, r = timed(lambda: s.fold_in(off, tok, w, iterations=ITERATIONS, seed=SEED, doc_base=D), calls)
        lines += [f"### {n} documents ({ntok} tokens, {ntok / n:.1f} a document over the views)", "",
                  f"- mvhdp_fold_in: {med:.1f} ms a call (first call {first:.1f} ms), of which the kernel {r.kernel_ms:.1f} ms; {r.visits} visits = "
                  f"{r.visits / r.kernel_ms / 1e6:.3f} G visits/s of kernel time, {r.visits / med / 1e6:.3f} G visits/s of wall time; "
                  f"{r.tokens} tokens in vocabulary ({r.oov} not)",
                  f"- device memory of the call: the chunk's buffers, at most 256 MiB, and the [M][2][64 T] table; theta comes back to the host "
                  f"({n * K * 8 / 2 ** 20:.0f} MiB)"]
        t0 = time.perf_counter()
        ms, theta2, held = second_handle_route(s, hy, K, V, off, tok, w)
        total = (time.perf_counter() - t0) * 1e3
        lines += [f"- the second-handle route, once: {total:.1f} ms in all: " + "; ".join(f"{k} {v:.1f} ms" for k, v in ms.items()),
                  "- device memory the second handle held: " + (f"{held / 2 ** 20:.0f} MiB" if held is not None else "not measured (no torch)"),
                  f"- mean |theta(fold_in) - theta(second handle)| over all cells: {float(np.abs(r.theta - theta2).mean()):.3e} "
                  f"(two chains of the same model, not the same bits); mean largest entry of a row: {float(r.theta.max(1).mean()):.4f} / {float(theta2.max(1).mean()):.4f}", ""]
        del r, theta2, nxt, off, tok
    s.close()
    head = open(args.out).read() if os.path.exists(args.out) else "# mvhdp_fold_in\n"
    marker = "\n## Measured: tools/foldin_timing.py"
    if marker in head:
        head = head[:head.index(marker)]
    open(args.out, "w").write(head.rstrip("\n") + "\n" + "\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
