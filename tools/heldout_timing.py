"""Cost of mvhdp_heldout_left_to_right at C4 on the state after the benchmark's window: the random start of bench.py, 25 deferred sweeps,
then 10 000 held-out documents, 10 particles, resample on and off.  Writes a markdown report (default profiles/heldout.md).

  python tools/heldout_timing.py [--workload C4] [--docs D] [--sweeps 25] [--heldout 10000] [--out profiles/heldout.md] [--no-profile]

Wall times are host clocks around the synchronous call (the method of profiles/phrases.md): four calls, the median of the last three.
Two inputs: documents of the same generator under another seed (other topic-word maps: the model has not seen their like), and the
generator's NEXT entities under the training seed (unseen documents of the training topics: the perplexity that means something).
Beside them: the chain's deferred sweep in tokens per second (the same row gather), and the sequential restatement tests/native/ltr_ref.c
on one host core, on the first documents of the first input.  Which unit the kernel leans on comes from two child runs of their own, one
under `rocprofv3 --kernel-trace --stats`, one under `rocprofv3 --pmc` (counters are never collected together with a trace).  The kernel's
cost does not depend on the count values (every visit reads a whole row), so the children evaluate on a model of the same shape trained
briefly on a cut of the corpus; no wall time is taken from them.  A child that exits with an error or does not end within its time limit
ends the profiling: its whole process group is killed, the report says so, and no further run is started on the GPU."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import SEED, ChildFailed, profiled, timed, trained_sampler  # noqa: E402

PARTICLES = 10
MI355X_CUS, MI355X_MAX_GHZ = 256, 2.4                                        # the chip the figures are read against
COUNTERS = ["SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_INSTS_VALU", "SQ_INSTS_VMEM_RD"]
KERNELS = r"heldout_\w+(<[\w, ]+>)?"


def heldout_inputs(workload, D, n):
    """view-0 documents: (another seed, the next n entities of the training seed)"""
    from mvtopicmodel_amd import synth
    c = dict(synth.CONFIGS[workload])
    other = synth.generate(c["K"], c["V"], n, c["lam"], c["seed"] ^ 0x48454C44, power_law_text=c.get("power_law_text", False))
    nxt = synth.generate(c["K"], c["V"], D + n, c["lam"], c["seed"], power_law_text=c.get("power_law_text", False), doc_lo=D, doc_hi=D + n)
    return (other.doc_off[0], other.tokens[0]), (nxt.doc_off[0], nxt.tokens[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C4")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--sweeps", type=int, default=25)
    ap.add_argument("--heldout", type=int, default=10000)
    ap.add_argument("--ref-docs", type=int, default=24, help="documents the host restatement evaluates (one particle)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heldout.md"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help="(internal) one resampling call, for the profiler")
    args = ap.parse_args()
    if args.child:
        s, _, _, D, _ = trained_sampler(args.workload, 50000, 2)
        (off, tok), _ = heldout_inputs(args.workload, D, args.heldout)
        s.heldout_left_to_right(off, tok, particles=PARTICLES, resample=True, seed=SEED)
        s.close()
        return
    s, hy, _, D, sweeps = trained_sampler(args.workload, args.docs, args.sweeps)
    sweep_ms, sweep_tokens = [x.total_ms for x in sweeps], sweeps[-1].tokens
    print(f"{args.sweeps} sweeps done", file=sys.stderr, flush=True)
    inputs = heldout_inputs(args.workload, D, args.heldout)
    sweep_med = statistics.median(sweep_ms[5:] or sweep_ms)
    lines = ["# mvhdp_heldout_left_to_right: timings", "",
             f"Written by tools/heldout_timing.py.  Workload {args.workload}" + (f" cut to {args.docs} entities" if args.docs else "") +
             f": K = {s.K}, V_0 = {s.V[0]}; the random start of bench.py, then {args.sweeps} deferred sweeps (seed {SEED}; median of sweeps 5.. "
             f"{sweep_med:.1f} ms on the device for {sweep_tokens} tokens = {sweep_tokens / sweep_med / 1e6:.2f} G tokens/s).",
             f"Held-out: {args.heldout} view-0 documents, {PARTICLES} particles.  Wall times: host clock around the synchronous call, the median of 3 calls after 1.", ""]
    visits_per_s = first_visits = None
    for name, (off, tok) in zip(["the generator under another seed (topic-word maps the model has not seen; the issue's input)",
                                 "the generator's next entities under the training seed (unseen documents of the training topics)"], inputs):
        lines += [f"## {name}", "", f"- {len(off) - 1} documents, {len(tok)} tokens, mean length {len(tok) / (len(off) - 1):.1f}, longest {int(np.diff(off).max())}"]
        for rs in (True, False):
            first, med, r = timed(lambda: s.heldout_left_to_right(off, tok, particles=PARTICLES, resample=rs, seed=SEED), n=4)
            lines.append(f"- resample {'on ' if rs else 'off'}: {med:.1f} ms a call (first call {first:.1f} ms); {r.visits} visits = {r.visits / med / 1e6:.3f} G visits/s; "
                         f"log-likelihood {r.log_likelihood:.6e}, {r.tokens} tokens in vocabulary ({r.oov} not), perplexity {r.perplexity:.1f}")
            if rs and visits_per_s is None:
                visits_per_s, first_visits = r.visits / med * 1e3, r.visits
            print(lines[-1], file=sys.stderr, flush=True)
        lines.append("")
    lines += ["## yardsticks", "",
              f"- the deferred sweep of this chain: {sweep_tokens / sweep_med / 1e6:.2f} G tokens/s; a token of the sweep and a visit here gather the same count row "
              f"(the sweep from the 16- or 12-bit mirror and only the entity's topic list; a visit all K cells of the 32-bit table and K weights in fp64)"]
    # the restatement on one host core
    from tests import ltr_ref as lr
    off, tok = inputs[0]
    n = min(args.ref_docs, len(off) - 1)
    nwk, nk = s.get_counts(0)
    alpha = s.get_alpha()[0][0, :s.K].copy()
    lr.lib()
    t0 = time.perf_counter()
    ref = lr.evaluate(nwk, nk, float(hy.beta[0]), alpha, float(hy.gamma[0] * hy.alpha_sum[0]), off[:n + 1], tok[:off[n]], particles=1, resample=True, seed=SEED)
    ref_s = time.perf_counter() - t0
    got = s.heldout_left_to_right(off[:n + 1], tok[:off[n]], particles=1, resample=True, seed=SEED, want_position_sums=True)
    same = bool(np.array_equal(got.position_sum, ref.S))
    lines += [f"- tests/native/ltr_ref.c (gcc -O2) on one host core, the first {n} documents, one particle: {ref.visits} visits in {ref_s * 1e3:.0f} ms = "
              f"{ref.visits / ref_s / 1e6:.4f} M visits/s; the device, resampling: {visits_per_s / 1e6:.0f} M visits/s = {visits_per_s / (ref.visits / ref_s):.0f} x; "
              f"position sums of those documents equal bit for bit: {same}", ""]
    s_K = s.K
    s.close()
    if not args.no_profile:
        child_argv = ["--workload", args.workload, "--heldout", str(args.heldout)]
        lines += ["## what the kernel leans on (two child runs of their own: a model of the same shape trained for 2 sweeps on 50 000 entities, one resampling call "
                  "on the first input)", ""]
        ks = pm = None
        try:                                                                 # a child that fails or hangs ends the profiling: nothing more goes to the GPU
            print("wall times taken; the kernel trace", file=sys.stderr, flush=True)
            ks = profiled(__file__, child_argv, KERNELS, limit=400)
            print("the counter pass", file=sys.stderr, flush=True)
            pm = profiled(__file__, child_argv, "heldout_ltr", mode="pmc", counters=COUNTERS, limit=400)
        except ChildFailed as e:
            lines += [f"- {e}; no further run was started", ""]
            print(f"{e}; no further run was started", file=sys.stderr, flush=True)
        ltr_ms = None
        if ks:
            lines += ["kernel trace (rocprofv3 --kernel-trace --stats):", ""]
            for name, (calls, ms) in sorted(ks.items(), key=lambda e: -e[1][1]):
                lines.append(f"- {name}: {ms:.2f} ms over {calls} launch(es)")
            lines.append("")
            ltr_ms = sum(ms for name, (_, ms) in ks.items() if "heldout_ltr" in name) or None
        else:
            lines += ["- no kernel trace (rocprofv3 is not installed, gave no kernel rows, or the run failed)", ""]
        if pm:
            lines += ["counters of the heldout_ltr_kernel dispatches (rocprofv3 --pmc, summed over the device; the SQ cycle counters tick once per four cycles):", ""]
            for c in COUNTERS:
                if c in pm:
                    lines.append(f"- {c}: {pm[c]:.4g}")
            wc = pm.get("SQ_WAVE_CYCLES")
            if wc:
                share = {c: pm[c] / wc for c in ("SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY") if c in pm}
                lines.append("- of the wave cycles (summed over waves): " + ", ".join(f"{c} {100 * v:.0f} %" for c, v in share.items()))
            if first_visits:                                                 # the child's call is the first input's resampling call
                per = {c: pm[c] / first_visits for c in ("SQ_INSTS_VALU", "SQ_INSTS_VMEM_RD") if c in pm}
                lines.append("- per visit: " + ", ".join(f"{c} {v:.1f}" for c, v in per.items()) + f"; a visit gathers {4 * s_K} bytes of counts")
            if ltr_ms and "SQ_ACTIVE_INST_VALU" in pm:
                simds = 4 * MI355X_CUS
                rate = 4 * pm["SQ_ACTIVE_INST_VALU"] / simds / (ltr_ms * 1e-3) / 1e9
                lines.append(f"- vector-ALU issue cycles per SIMD ({simds} SIMDs) over the traced kernel time: {rate:.2f} G cycles/s against a clock of at most "
                             f"{MI355X_MAX_GHZ} GHz = at least {100 * rate / MI355X_MAX_GHZ:.0f} % of the SIMD's time")
                if first_visits:
                    lines.append(f"- count bytes gathered over the traced kernel time: {4 * s_K * first_visits / (ltr_ms * 1e-3) / 1e12:.2f} TB/s over the device")
            lines.append("")
        else:
            lines += ["- no counters (rocprofv3 is not installed, gave no rows for the kernel, or a run failed)", ""]
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
