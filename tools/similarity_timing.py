"""Cost of mvhdp_similar_pairs at the sizes of the flow's calcSimilarities: dim = 400, n = 20 000 and 100 000 synthetic entity vectors,
threshold 0.15, min_weight 0.03, metric COS_FOLDED.  Writes a markdown report (default profiles/similarity.md).

  python tools/similarity_timing.py [--sizes 20000,100000] [--dim 400] [--out profiles/similarity.md] [--no-profile]

Wall times are host clocks around the synchronous call.  Kernel times come from a second run of the same call under
`rocprofv3 --kernel-trace --stats` (a child process of its own; tracing slows the host, so no wall time is taken from it).  The screen's
rate is 2 * dim * pairs_screened / (sum of the screen kernel's durations): the cells the launched tiles compute, ragged edges and
diagonal tiles included, at the useful dim (the kernel itself runs dim padded to a multiple of 32).  The numpy restatement
(tests/sim_numpy.py) is timed at n = 2 000 for scale, and the JSD's largest deviation from it is recorded on the shapes of the test."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_F32_MFMA_TF = 155.0        # MI355X fp32-input MFMA peak
GUIDE_UNTUNED_TF = 122.0        # an untuned 128 x 128 x 32 LDS-tiled kernel on the same instruction, 4096^3
THRESHOLD, MIN_WEIGHT = 0.15, 0.03


NOTES = ["## Reading the figures", "",
         "- The screen's rate counts 2 * 400 flops for every cell of every launched tile.  The kernel itself multiplies 416 columns (dim padded to",
         "  the 32-wide k-slab: 4 % more work than counted) and each stripe's launch ends in a tail of partly filled CUs.  What else may keep it below",
         "  the untuned 4096^3 figure (none of it measured separately): one LDS buffer with two block barriers per k-slab and no software pipelining beyond the global loads of",
         "  the next slab, at two blocks a CU; dim = 400 is 13 slabs, so the 64-register accumulator is set up and the 128 x 128 epilogue",
         "  (class lookups, two passes of 64 ballots, one atomic a block) is paid once per 13 slabs instead of once per 128.",
         "- The first version of the epilogue appended with one atomic per ballot on the stripe's single counter (tens of millions of them at n = 100 000):",
         "  452 ms for the screen (8.9 TFLOP/s).  Counting per block first and taking the block's room with one atomic gave the figures above.",
         "- The exact stage reads two rows of 3.2 KB per candidate, a lane walking its own pair of rows: every load instruction of a wave touches",
         "  up to 64 cache lines whatever its width.  16-byte loads (two entries a load; rows of even dim) took it from 171.6 to 38.0 ms at",
         "  n = 100 000, which points at cache-line throughput rather than fp64 arithmetic (no counters were taken).",
         "- The call that returns the pairs is host-bound: 51.5 M survivors are copied back, sorted by key per stripe and split into three arrays",
         "  (about 2.7 s of the 2.77 s).  The count-only call shows the device's share.", ""]


def entity_vectors(n, dim, seed=1):
    """rows like the flow's entity distributions: one dominant topic (0.3 .. 0.6), two to six minor ones (0.03 .. 0.1), the rest 0"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, dim))
    x[np.arange(n), rng.integers(0, dim, n)] = rng.uniform(0.3, 0.6, n)
    for _ in range(6):
        on = rng.random(n) < 0.7
        rows = np.flatnonzero(on)
        x[rows, rng.integers(0, dim, len(rows))] = rng.uniform(0.031, 0.1, len(rows))
    return x


def run_call(s, x, count_only):
    from mvtopicmodel_amd import _lib
    a = _lib.SimArgsC(0, x.shape[0], x.shape[1], x.ctypes.data, MIN_WEIGHT, THRESHOLD, 0, 0)
    cnt, st = C.c_int64(), _lib.SimStatsC()
    t0 = time.perf_counter()
    rc = s.L.mvhdp_similar_pairs(s.h, C.byref(a), 0, None, None, None, C.byref(cnt), C.byref(st))
    t_count = time.perf_counter() - t0
    assert rc == 0, s.L.mvhdp_last_error(s.h)
    out = dict(count=cnt.value, count_only_s=t_count, pairs_screened=st.pairs_screened, candidates=st.candidates, emitted=st.emitted,
               stripes=st.stripes, regrown=st.regrown, margin=st.margin)
    if not count_only:
        n = cnt.value
        i, j, v = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n)
        t0 = time.perf_counter()
        rc = s.L.mvhdp_similar_pairs(s.h, C.byref(a), n, i.ctypes.data, j.ctypes.data, v.ctypes.data, C.byref(cnt), C.byref(st))
        out["full_s"] = time.perf_counter() - t0
        assert rc == 0 and cnt.value == n
        out["regrown_full"] = st.regrown
    return out


def kernel_times(directory):
    """{kernel name: (calls, total ns)} from whatever rocprofv3 left under `directory`"""
    out = {}
    for f in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Name") or r.get("KernelName") or ""
            out[name] = (int(r.get("Calls", 0)), float(r.get("TotalDurationNs", 0)))
    if out:
        return out
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Kernel_Name", "")
            c, t = out.get(name, (0, 0.0))
            out[name] = (c + 1, t + float(r["End_Timestamp"]) - float(r["Start_Timestamp"]))
    return out


def child(n, dim):
    from mvtopicmodel_amd import NativeSampler
    with NativeSampler(4, [8]) as s:
        print(json.dumps(run_call(s, entity_vectors(n, dim), True)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20000,100000")
    ap.add_argument("--dim", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similarity.md"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.dim)
    from mvtopicmodel_amd import NativeSampler
    from tests import sim_numpy as sn
    lines = ["# mvhdp_similar_pairs: timings", "",
             f"Written by tools/similarity_timing.py.  dim = {a.dim}, metric COS_FOLDED, threshold {THRESHOLD}, min_weight {MIN_WEIGHT}; synthetic entity",
             "vectors (one dominant topic, two to six minor ones).  Wall times: host clock around the synchronous call, second call of that shape",
             "in the process.  Kernel times: a separate run under `rocprofv3 --kernel-trace --stats`.", ""]
    with NativeSampler(4, [8]) as s:
        run_call(s, entity_vectors(512, a.dim), False)                       # code objects loaded, buffers touched
        for n in [int(v) for v in a.sizes.split(",") if v]:
            x = entity_vectors(n, a.dim)
            run_call(s, x[:2048], True)
            r = run_call(s, x, False)
            lines += [f"## n = {n}", "",
                      f"- pairs emitted: {r['emitted']}; candidates: {r['candidates']} (candidates / emitted = {r['candidates'] / max(r['emitted'], 1):.3f}); "
                      f"cells screened: {r['pairs_screened']}; stripes: {r['stripes']}; stripes redone with a larger buffer: {r['regrown']}",
                      f"- wall, count-only call: {r['count_only_s'] * 1e3:.1f} ms; wall, call that returns the pairs: {r['full_s'] * 1e3:.1f} ms "
                      f"(host-side sort and copy of {r['emitted']} pairs included)"]
            print(json.dumps(dict(n=n, **r)), flush=True)
            if not a.no_profile:
                d = tempfile.mkdtemp(prefix=f"sim_prof_{n}_")
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
                       "--child", str(n), "--dim", str(a.dim)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                kt = kernel_times(d) if p.returncode == 0 else {}
                if not kt:
                    lines.append(f"- kernel times: not measured (rocprofv3 exit {p.returncode}: {p.stderr.strip()[-300:]})")
                else:
                    pick = lambda key: sum(t for k, (c, t) in kt.items() if key in k)
                    screen, exact, total = pick("sim_screen_kernel"), pick("sim_exact_kernel"), sum(t for c, t in kt.values())
                    tf = 2.0 * a.dim * r["pairs_screened"] / screen / 1e3 if screen else float("nan")
                    lines += [f"- screen kernel: {screen / 1e6:.2f} ms over {r['stripes']} launches = {tf:.1f} TFLOP/s at the useful dim "
                              f"({100 * tf / PEAK_F32_MFMA_TF:.0f} % of the {PEAK_F32_MFMA_TF:.0f} TF fp32-MFMA peak, {100 * tf / GUIDE_UNTUNED_TF:.0f} % of the "
                              f"{GUIDE_UNTUNED_TF:.0f} TF an untuned tile kernel reaches at 4096^3)",
                              f"- exact stage: {exact / 1e6:.2f} ms = {100 * exact / total:.1f} % of all kernel time ({total / 1e6:.2f} ms); "
                              f"prepare + normalise: {(pick('sim_prepare_kernel') + pick('sim_normalise_kernel')) / 1e6:.2f} ms"]
                    print(json.dumps({k: v for k, v in kt.items()}), flush=True)
            lines.append("")
        # the restatement, for scale
        x = entity_vectors(2000, a.dim)
        t0 = time.perf_counter()
        want = sn.similar_pairs(x, sn.COS_FOLDED, THRESHOLD, MIN_WEIGHT)
        t_np = time.perf_counter() - t0
        got = s.similar_pairs(x, sn.COS_FOLDED, THRESHOLD, MIN_WEIGHT)
        same = np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()
        lines += ["## for scale", "", f"- numpy restatement (tests/sim_numpy.py) at n = 2000: {t_np:.2f} s for {len(want[0])} pairs; the device's result is "
                  f"{'bit-identical' if same else 'DIFFERENT'}", ""]
        # JSD: largest deviation from the restatement on the shapes of tests/test_gpu_similarity.py
        from tests.test_gpu_similarity import prob_rows
        worst = 0.0
        for n, dim in [(2, 3), (33, 2), (33, 33), (129, 100), (300, 33), (40, 400)]:
            p = prob_rows(n, dim, 50 + n + dim)
            gi, gj, gv, _ = s.similar_pairs(p, sn.JSD, 0.02)
            wi, wj, wv = sn.similar_pairs(p, sn.JSD, 0.02)
            assert np.array_equal(gi, wi) and np.array_equal(gj, wj)
            worst = max(worst, float(np.abs(gv - wv).max()) if len(gv) else 0.0)
        lines += ["## JSD", "", f"- largest |device - restatement| over the shapes of tests/test_gpu_similarity.py (threshold 0.02): {worst:.3e} "
                  f"(the test's bound at dim = 100 for rows that sum to 1: {8 * 100 * 2.0 ** -52 * 2:.3e})", ""]
    lines += NOTES
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
