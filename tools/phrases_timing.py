"""Cost of mvhdp_topic_phrases at C4 on the state after the benchmark's window: the random start of bench.py, 25 deferred sweeps, then
max_per_topic = 20.  Writes a markdown report (default profiles/phrases.md).

  python tools/phrases_timing.py [--workload C4] [--docs D] [--sweeps 25] [--out profiles/phrases.md] [--no-profile]

Wall times are host clocks around the synchronous call (the method of profiles/similarity.md): six calls, the median of the last five.
In the same process, as yardsticks: mvhdp_diagnostics (N = 20), which also walks the view-0 tokens, and mvhdp_get_assignments of view 0,
the floor of any host-side path.  Kernel times come from a second run of the same state under `rocprofv3 --kernel-trace --stats` (a child
process of its own; no wall time is taken from it).  The extra device memory is computed from the sizes the call reports (the buffers of
mvhdp_phrases.hip are sized by them), not sampled."""
import argparse
import csv
import ctypes as C
import glob
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _timing import SEED, timed, trained_sampler  # noqa: E402


NOTES = ["## Reading the figures", "",
         "- The first version of the write pass took its room with one atomic per 64-position step on a single counter (about ten million of them at",
         "  C4): 27.55 ms for that kernel against 0.69 ms for the count pass that walks the same tokens, and 58 ms for the whole call.  The count",
         "  pass now leaves every wave's number of occurrences, the host turns the few thousand numbers into offsets between the two passes",
         "  (it waits there anyway, for the total), and the same grid writes without an atomic.",
         "- Where the rest goes: the count by key is one scattered atomic per occurrence plus the compare on the corpus, the scatter one atomic",
         "  per distinct phrase on K cursors; the select pass reads a topic's segment once per bit of its largest count.  The difference between",
         "  the kernels' sum and the wall time is the host side of one call -- a dozen hipMalloc / hipFree of up to several hundred MiB, three",
         "  memsets of the table, five synchronisations -- none of it measured separately.  A host that calls this once after training pays",
         "  it once; a buffer kept on the handle would remove it and was not built (the issue asks for no cache).",
         "- max_per_topic = -1 is host-bound: every distinct phrase crosses and the host sorts them by count and word ids.", ""]


def phrase_call(s, max_n, sizes=None):
    from mvtopicmodel_amd import _lib
    a = _lib.PhraseArgsC(max_n, 0)
    n, w, st = C.c_int64(), C.c_int64(), _lib.PhraseStatsC()
    if sizes is None:
        rc = s.L.mvhdp_topic_phrases(s.h, C.byref(a), 0, 0, None, None, None, None, None, None, C.byref(n), C.byref(w), C.byref(st))
    else:
        arr = [np.zeros(s.K + 1, np.int64), np.zeros(sizes[0] + 1, np.int64), np.zeros(max(sizes[1], 1), np.int32), np.zeros(max(sizes[0], 1), np.int32),
               np.zeros(s.K, np.int64), np.zeros(s.K, np.int64)]
        rc = s.L.mvhdp_topic_phrases(s.h, C.byref(a), sizes[0], sizes[1], *[x.ctypes.data for x in arr], C.byref(n), C.byref(w), C.byref(st))
    assert rc == 0, s.L.mvhdp_last_error(s.h)
    return n.value, w.value, st


def kernel_stats(argv):
    """{kernel name: (calls, total ms)} of a child run under rocprofv3, or None"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "phrases", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__)] + argv + ["--child"]
        try:
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=420)
        except (OSError, subprocess.SubprocessError):
            return None
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        out = {}
        for row in csv.DictReader(open(files[0])):
            m = re.search(r"phrase_\w+(<\w+>)?", row["Name"])
            if m:
                out[m.group(0)] = (int(row["Calls"]), float(row["TotalDurationNs"]) / 1e6)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C4")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--sweeps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phrases.md"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", action="store_true", help="(internal) one call of each kind, for the kernel trace")
    args = ap.parse_args()
    s, _, corpus, _, sweeps = trained_sampler(args.workload, args.docs, args.sweeps)
    sweep_ms, n0 = [x.total_ms for x in sweeps], int(corpus.doc_off[0][-1])
    print(f"{args.sweeps} sweeps done", file=sys.stderr, flush=True)
    if args.child:
        phrase_call(s, 20)
        s.close()
        return
    first_q, med_q, _ = timed(lambda: phrase_call(s, 20), n=6)
    np_, nw, st = phrase_call(s, 20)
    first_f, med_f, _ = timed(lambda: phrase_call(s, 20, (np_, nw)), n=6)
    _, med_all, _ = timed(lambda: phrase_call(s, -1), n=3)
    _, med_diag, _ = timed(lambda: s.diagnostics(20), n=6)
    _, med_z, _ = timed(lambda: s.get_assignments(0), n=6)
    cap = 64
    while cap < 2 * st.occurrences:
        cap *= 2
    extra = 24 * st.occurrences + 12 * cap + 12 * st.distinct
    lines = ["# mvhdp_topic_phrases: timings", "",
             f"Written by tools/phrases_timing.py.  Workload {args.workload}" + (f" cut to {args.docs} entities" if args.docs else "") +
             f": {n0} view-0 tokens, K = {s.K}; the random start of bench.py, then {args.sweeps} deferred sweeps (seed {SEED}; the last one took {sweep_ms[-1]:.1f} ms on the device, the median {statistics.median(sweep_ms):.1f} ms).",
             "Wall times: host clock around the synchronous call, the median of 5 calls after 1.", "",
             "## max_per_topic = 20", "",
             f"- the size query (arrays NULL): {med_q:.1f} ms (first call {first_q:.1f} ms); the call that fills the arrays: {med_f:.1f} ms (first call {first_f:.1f} ms); the Python wrapper makes both",
             f"- runs: {st.runs}; occurrences: {st.occurrences}; distinct: {st.distinct}; kept: {st.kept} phrases, {nw} words; hash collisions at 64 bits: {st.hash_collisions}",
             f"- extra device memory at the peak (records 24 B x occurrences, table 12 B x {cap} slots, per-topic segments 12 B x distinct): {extra / 2 ** 20:.0f} MiB",
             f"- max_per_topic = -1 (every phrase, what a merge of shards asks for; the host sorts all of them), size query: {med_all:.1f} ms", "",
             "## yardsticks, the same process and state", "",
             f"- mvhdp_diagnostics (N = 20), which also walks the view-0 tokens: {med_diag:.1f} ms",
             f"- mvhdp_get_assignments of view 0 ({4 * n0 / 2 ** 20:.0f} MiB to the host), the floor of any host-side path: {med_z:.1f} ms",
             f"- one deferred sweep of this chain: {statistics.median(sweep_ms):.1f} ms", ""]
    s.close()
    if not args.no_profile:
        print("wall times taken; the kernel trace", file=sys.stderr, flush=True)
        ks = kernel_stats([a for a in sys.argv[1:] if a != "--no-profile"])
        if ks:
            lines += ["## kernels of one size query (rocprofv3 --kernel-trace --stats, a run of its own)", ""]
            for name, (calls, ms) in sorted(ks.items(), key=lambda e: -e[1][1]):
                lines.append(f"- {name}: {ms:.2f} ms over {calls} launch(es)")
            lines += [f"- together: {sum(ms for _, ms in ks.values()):.2f} ms of the {med_q:.1f} ms the call takes", ""]
    lines += NOTES
    open(args.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
