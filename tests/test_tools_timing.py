"""The child runner of the timing reports (tools/_timing.py: profiled) against stand-ins for rocprofv3: executables of that name put first
on PATH.  It is the protocol that is checked -- what is started and how, what happens to the child's process group when the child fails
or outstays its limit, which rows of the profiler's tables come back -- with no GPU and no profiler."""
import json
import os
import stat
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _timing  # noqa: E402

KERNELS = r"xe_\w+|xview_score_kernel"
STATS = """"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"
"void xe_pick_kernel<true>(XePick)",3,1500000,500000,10.0,1,2,0.1
"void xe_pick_kernel<false>(XePick)",2,500000,250000,10.0,1,2,0.1
"xview_score_kernel(double const*, int)",1,4000000,4000000,70.0,1,2,0.1
"mvhdp_sweep_kernel(SweepArgs)",50,9000000,180000,10.0,1,2,0.1
"""
COUNTS = """"Dispatch_Id","Kernel_Name","Counter_Name","Counter_Value"
1,"xview_score_kernel(double const*, int)","SQ_WAVE_CYCLES",100.5
2,"xview_score_kernel(double const*, int)","SQ_WAVE_CYCLES",50
2,"xview_score_kernel(double const*, int)","SQ_INSTS_VALU",7
3,"xview_phi_kernel(int)","SQ_WAVE_CYCLES",1000
"""


@pytest.fixture
def standin(tmp_path, monkeypatch):
    """standin(body): an executable rocprofv3 first on PATH that runs `body` (python; argv and `log`, a file of the test's, are at hand)"""
    bindir = tmp_path / "bin"
    bindir.mkdir()
    log = tmp_path / "log.json"
    monkeypatch.setenv("PATH", str(bindir) + os.pathsep + os.environ["PATH"])

    def make(body):
        exe = bindir / "rocprofv3"
        exe.write_text(f"#!{sys.executable}\nimport json, os, subprocess, sys, time\nargv, log = sys.argv[1:], {str(log)!r}\n{body}\n")
        exe.chmod(exe.stat().st_mode | stat.S_IXUSR)
        return log
    return make


def gone(pid):
    """no such process, or one that has ended and only waits for whoever collects orphans"""
    try:
        return open(f"/proc/{pid}/stat").read().rsplit(")", 1)[1].split()[0] == "Z"
    except FileNotFoundError:
        return True


def test_a_failing_child_is_reported_with_its_status(standin):
    standin("sys.exit(3)")
    with pytest.raises(_timing.ChildFailed, match="status 3"):
        _timing.profiled("report.py", [], KERNELS)


def test_a_child_past_its_limit_is_killed_with_its_group(standin):
    log = standin("g = subprocess.Popen([sys.executable, '-c', 'import time; time.sleep(60)'])\n"
                  "json.dump([os.getpid(), g.pid, os.getpgid(0), os.getpgid(g.pid)], open(log + '.part', 'w'))\nos.rename(log + '.part', log)\ntime.sleep(60)")
    t0 = time.monotonic()
    with pytest.raises(_timing.ChildFailed, match="did not end within 1 s"):
        _timing.profiled("report.py", [], KERNELS, limit=1)
    assert time.monotonic() - t0 < 10.0
    child, grandchild, group, group_of_grandchild = json.load(open(log))
    assert group == child == group_of_grandchild != os.getpgid(0)            # a group of its own, the profiled program in it
    end = time.monotonic() + 5.0
    while not gone(grandchild) and time.monotonic() < end:                  # (SIGKILL is on its way to the orphan; the child itself was reaped)
        time.sleep(0.01)
    assert gone(child) and gone(grandchild)
    with pytest.raises(ProcessLookupError):
        os.kill(child, 0)


def test_a_trace_returns_the_matching_kernels_summed(standin):
    log = standin("json.dump(argv, open(log, 'w'))\nd = os.path.join(argv[argv.index('-d') + 1], 'host', '4242')\nos.makedirs(d)\n"
                  f"open(os.path.join(d, '4242_kernel_stats.csv'), 'w').write({STATS!r})")
    got = _timing.profiled("some/report.py", ["--workload", "C4"], KERNELS, limit=20)
    assert set(got) == {"xe_pick_kernel", "xview_score_kernel"}
    assert got["xe_pick_kernel"] == (5, pytest.approx(2.0)) and got["xview_score_kernel"] == (1, pytest.approx(4.0))
    argv = json.load(open(log))
    head, program = argv[:argv.index("--")], argv[argv.index("--") + 1:]
    assert "--kernel-trace" in head and "--stats" in head and "--pmc" not in argv
    assert program == [sys.executable, os.path.abspath("some/report.py"), "--workload", "C4", "--child"]


def test_a_counter_run_is_a_run_of_its_own(standin):
    log = standin("json.dump(argv, open(log, 'w'))\nd = argv[argv.index('-d') + 1]\n"
                  f"open(os.path.join(d, 'run_counter_collection.csv'), 'w').write({COUNTS!r})")
    got = _timing.profiled("report.py", [], "xview_score_kernel", mode="pmc", counters=["SQ_WAVE_CYCLES", "SQ_INSTS_VALU"], limit=20)
    assert got == {"SQ_WAVE_CYCLES": pytest.approx(150.5), "SQ_INSTS_VALU": pytest.approx(7.0)}
    argv = json.load(open(log))
    head = argv[:argv.index("--")]
    assert head[:3] == ["--pmc", "SQ_WAVE_CYCLES", "SQ_INSTS_VALU"] and "--kernel-trace" not in argv and "--stats" not in argv
    assert not any("trace" in a for a in head)


def test_nothing_to_report_is_none(standin, tmp_path, monkeypatch):
    standin("pass")                                                          # a run that ends well and leaves no table
    assert _timing.profiled("report.py", [], KERNELS, limit=20) is None
    standin(f"d = argv[argv.index('-d') + 1]\nopen(os.path.join(d, 'x_kernel_stats.csv'), 'w').write({STATS!r})")
    assert _timing.profiled("report.py", [], r"gram_\w+", limit=20) is None  # a table without a matching row
    empty = tmp_path / "empty"
    empty.mkdir()
    monkeypatch.setenv("PATH", str(empty))                                   # no rocprofv3: nothing is started
    assert _timing.profiled("report.py", [], KERNELS, limit=20) is None
