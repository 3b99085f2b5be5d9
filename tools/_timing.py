"""What the side calls' timing reports (tools/*_timing.py) share: the trained model they measure on, the host clock around a call, the
compiler's resource figures of a unit's kernels, and the one way a report starts a child run under rocprofv3.  A child that fails or
runs into its time limit ends the profiling: its process group is killed and reaped, and ChildFailed tells the report to start nothing
more on the GPU."""
import csv
import glob
import os
import re
import shutil
import signal
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SEED = 20260101                                                              # bench.py's
# CXXFLAGS of mvtopicmodel_amd/csrc/Makefile, without -fPIC and the warning switches: what decides the code the kernels become
KERNEL_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mllvm", "-structurizecfg-skip-uniform-regions=1"]
RESOURCES = r"(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)"


def trained_sampler(workload, docs, sweeps):
    """The random start of bench.py on `docs` entities of the workload (None: all of them), then `sweeps` deferred sweeps:
    (sampler, hyper, corpus, D, the sweeps' statistics)."""
    from mvtopicmodel_amd import NativeSampler, synth
    from mvtopicmodel_amd.java_init import init_assignments
    from mvtopicmodel_amd.native import Hyper
    cfg = dict(synth.CONFIGS[workload])
    D = docs or cfg["D"]
    K, V = cfg["K"], cfg["V"]
    corpus = synth.make_config(workload, D=D, doc_lo=0, doc_hi=D)
    inactive, K_init = synth.config_inactive(workload)
    z0 = init_assignments(K_init, corpus.doc_off, seed=1)
    s = NativeSampler(K, V)
    for m in range(len(V)):
        s.set_corpus(m, corpus.doc_off[m], corpus.tokens[m])
        s.set_assignments(m, z0[m])
    hy = Hyper.defaults(K, V, inactive=inactive)
    s.set_hyper(hy)
    s.build_counts()
    return s, hy, corpus, D, [s.sweep(i, SEED) for i in range(sweeps)]


def weights_without(M, m):
    w = np.ones(M)
    if M > 1:
        w[m] = 0.0
    return w


def timed(f, n=3):
    """n calls: (ms of the first, median ms of the others, the last result)"""
    out, r = [], None
    for _ in range(n):
        t0 = time.perf_counter()
        r = f()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[0], statistics.median(out[1:]), r


def resource_usage(source, kernel_pattern):
    """[(mangled function name, the kernel's name by kernel_pattern, {figure: value})] of the kernels of mvtopicmodel_amd/csrc/<source>
    that match, from a device-only compile: registers, scratch, occupancy, LDS.  Empty without hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return []
    r = subprocess.run([hipcc] + KERNEL_FLAGS + ["-S", "--cuda-device-only", "-o", os.devnull, os.path.join(ROOT, "mvtopicmodel_amd", "csrc", source),
                                                 "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    out, mangled, name, got = [], None, None, {}
    for l in r.stderr.split("\n"):
        f = re.search(r"Function Name: (\S+)", l)
        if f:
            mangled = f.group(1)
            k = re.search(kernel_pattern, mangled)
            name, got = (k.group(0) if k else None), {}
        elif name:
            v = re.search(RESOURCES, l)
            if v:
                got[v.group(1)] = v.group(2)
                if v.group(1).startswith("LDS"):                             # (the last figure of a function's remarks)
                    out.append((mangled, name, got))
                    name = None
    return out


def resource_lines(source, kernel_pattern, label=lambda name, mangled: name):
    """one line a kernel: its name (as `label` writes it) and the figures"""
    return [f"{label(name, mangled)}: " + ", ".join(f"{a} {b}" for a, b in got.items()) for mangled, name, got in resource_usage(source, kernel_pattern)]


class ChildFailed(RuntimeError):
    """a profiled child run ended with a non-zero status or ran into its time limit: nothing more is started on the GPU in this call"""


def profiled(script, argv, kernels, mode="trace", counters=None, limit=300):
    """`script` argv --child under rocprofv3, in a process group of its own.  mode 'trace' (--kernel-trace --stats) -> {kernel: (calls,
    total ms)}, summed over the rows whose name matches the pattern `kernels` and keyed by the match; mode 'pmc' (--pmc with `counters`,
    never in one run with a trace) -> {counter: sum over the dispatches whose kernel name contains the string `kernels`}.  None when
    rocprofv3 is not installed (nothing was started) or its output has no such rows.  ChildFailed when the child exits with a non-zero
    status (a fault, an abort) or does not end within `limit` seconds; the whole group -- rocprofv3 and the python process under it that
    holds the GPU -- is killed and reaped before that is raised."""
    if shutil.which("rocprofv3") is None:
        return None
    with tempfile.TemporaryDirectory() as d:
        what = ["--kernel-trace", "--stats"] if mode == "trace" else ["--pmc"] + list(counters)
        cmd = ["rocprofv3"] + what + ["-d", d, "-o", "run", "--output-format", "csv", "--", sys.executable, os.path.abspath(script)] + argv + ["--child"]
        child = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
        try:
            rc = child.wait(timeout=limit)
        except subprocess.TimeoutExpired:
            rc = None
        if rc != 0:
            try:
                os.killpg(child.pid, signal.SIGKILL)                         # the session leader's pid is the group's
            except ProcessLookupError:
                pass
            child.wait()
            raise ChildFailed(f"the {mode} run " + ("did not end within %d s" % limit if rc is None else "ended with status %d" % rc))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv" if mode == "trace" else "*counter_collection.csv"), recursive=True)
        if not files:
            return None
        out = {}
        for row in csv.DictReader(open(files[0])):
            if mode == "trace":
                k = re.search(kernels, row["Name"])
                if k:
                    calls, ms = out.get(k.group(0), (0, 0.0))
                    out[k.group(0)] = (calls + int(row["Calls"]), ms + float(row["TotalDurationNs"]) / 1e6)
            elif kernels in row.get("Kernel_Name", ""):
                out[row["Counter_Name"]] = out.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
        return out or None
