"""What the useVectorsLambda mix (mvhdp_set_vectors_mix) costs, and that switching it off costs nothing.  One JSON line per measurement.

  python tools/mix_timing.py cost [--workload C4] [--settle 40] [--reps 5] [--lam 0.25] [--lib build_var/libmvhdp_NAME.so]
      one handle, deferred sweeps from the addInstances start: `settle` sweeps, then blocks of `reps` sweeps alternating lambda = 0 and
      lambda = 0.25 (off, on, off, on) -- sweep-kernel ms and tokens/s of every block,
      set_vectors_mix itself (the host-side check, the upload and the table pass) and the tree rebuild with the mix against without.
  python tools/mix_timing.py off --other-tree DIR [--rounds 5] [--steps 20] [--warmup 5]
      bench.py's C4 deferred window in this tree and in another checkout of the project (the parent commit, built), one fresh process
      each, alternating: both sets of runs, so that the difference can be held against either tree's own run-to-run spread.

Times are device events (sweep_kernel_ms) or a host clock around calls that end in a synchronise."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def low_rank_table(K, V0, seed, rank=4):
    rng = np.random.RandomState(seed)
    dot = rng.standard_normal((K, rank)) @ rng.standard_normal((rank, V0))
    e = np.exp(dot - dot.max(axis=1, keepdims=True))
    return e, e.sum(axis=1)


def cost(a):
    from mvtopicmodel_amd import _lib
    if a.lib:                                                        # another build of the library (make -C mvtopicmodel_amd/csrc var NAME=... EXTRA=...)
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from mvtopicmodel_amd import NativeSampler, synth
    from mvtopicmodel_amd.java_init import init_assignments
    from mvtopicmodel_amd.native import Hyper
    cfg = synth.CONFIGS[a.workload]
    K, V = cfg["K"], cfg["V"]
    M = len(V)
    c = synth.make_config(a.workload)
    _, K_init = synth.config_inactive(a.workload)
    z0 = init_assignments(K_init, c.doc_off, seed=1)
    e, S = low_rank_table(K, V[0], 11)
    view0 = int(c.doc_off[0][-1]) / c.total_tokens
    with NativeSampler(K, V) as s:
        for m in range(M):
            s.set_corpus(m, c.doc_off[m], c.tokens[m]); s.set_assignments(m, z0[m])
        s.set_hyper(Hyper.defaults(K, V)); s.build_counts()
        s.sweep_many(0, a.settle, a.seed)
        print(json.dumps({"what": "setup", "lib": os.path.basename(a.lib) if a.lib else "libmvhdp.so", "workload": a.workload, "K": K, "V0": V[0], "tokens": c.total_tokens, "view0_token_share": round(view0, 4),
                          "settle_sweeps": a.settle, "mix_table_mb": round(8.0 * K * V[0] / 1e6, 1)}), flush=True)
        idx = a.settle
        for block, lam in enumerate([0.0, a.lam, 0.0, a.lam]):
            t0 = time.perf_counter()
            s.set_vectors_mix(lam, e if lam else None, S if lam else None)
            set_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            s.build_trees()                                          # (synchronous: the FTree.tree arrays and the descent tables of every row)
            trees_ms = (time.perf_counter() - t0) * 1e3
            s.sweep(idx, a.seed); idx += 1                           # (the flavours' first launch, the walk search's first proposal)
            km, tm, fb = [], [], 0
            for _ in range(a.reps):
                st = s.sweep(idx, a.seed); idx += 1
                km.append(st.sweep_kernel_ms); tm.append(st.total_ms); fb += st.exact_fallbacks
            print(json.dumps({"what": "block", "block": block, "lambda": lam, "set_vectors_mix_ms": round(set_ms, 2), "build_trees_full_ms": round(trees_ms, 3),
                              "sweep_kernel_ms": [round(x, 3) for x in km], "sweep_kernel_ms_median": round(float(np.median(km)), 3),
                              "total_ms_median": round(float(np.median(tm)), 3), "tokens_per_s": round(c.total_tokens / (float(np.median(tm)) / 1e3)),
                              "exact_fallbacks": fb, "first_sweep": idx - a.reps}), flush=True)


def off(a):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup", str(a.warmup), "--no-cpu-baseline", "--live-steps", "0"]
    trees = [("this", ROOT), ("other", os.path.abspath(a.other_tree))]
    got = {n: [] for n, _ in trees}
    kms = {n: [] for n, _ in trees}
    for r in range(a.rounds):
        for name, d in (trees if r % 2 == 0 else trees[::-1]):
            p = subprocess.run(cmd, cwd=d, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:                                    # (a run that fails ends the measurement: nothing more is started)
                print(json.dumps({"what": "bench_failed", "tree": name, "rc": p.returncode, "stderr": p.stderr[-400:]}), flush=True)
                sys.exit(1)
            out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            got[name].append(out["value"])
            kms[name].append(out.get("roofline", {}).get("avg_kernel_ms"))
            print(json.dumps({"what": "bench", "tree": name, "round": r, "value": out["value"], "unit": out.get("unit"), "ms_per_step": out.get("ms_per_step"),
                              "avg_kernel_ms": kms[name][-1], "final_nk_fingerprint": out.get("final_nk_fingerprint")}), flush=True)
    summ = {n: {"runs": v, "median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "spread": float(max(v) - min(v)),
                "avg_kernel_ms": kms[n]} for n, v in got.items()}
    summ["this_over_other_median"] = summ["this"]["median"] / summ["other"]["median"]
    # inside the other tree's own run-to-run spread: this tree's median between the other's slowest and fastest run
    summ["this_median_inside_others_range"] = bool(summ["other"]["min"] <= summ["this"]["median"] <= summ["other"]["max"])
    print(json.dumps({"what": "summary", **summ}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("cost")
    c.add_argument("--workload", default="C4"); c.add_argument("--settle", type=int, default=40); c.add_argument("--reps", type=int, default=5)
    c.add_argument("--lib", default=None); c.add_argument("--lam", type=float, default=0.25); c.add_argument("--seed", type=int, default=20260101)
    o = sub.add_parser("off")
    o.add_argument("--other-tree", required=True); o.add_argument("--rounds", type=int, default=5); o.add_argument("--steps", type=int, default=20)
    o.add_argument("--warmup", type=int, default=5); o.add_argument("--timeout", type=int, default=400)
    a = ap.parse_args()
    (cost if a.cmd == "cost" else off)(a)


if __name__ == "__main__":
    main()
