"""tools/steps.py, the step runner and timer the operator timing tools share: trouble in one step ends the run, the trace
step's command line, the orchestrators stay off the GPU, the reader of rocprofv3's kernel statistics, the out-of-memory
path of the largest-batch loop -- all on the host, with a throw-away tool whose steps are plain Python -- and the events
timer on the GPU."""
import os
import subprocess
import sys
import time
import weakref

import pytest
import torch

from tools import fape_time, steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ("irg_backward_time", "nerf_backward_time", "fape_time", "lddt_time", "violation_time")

# a tool as the runner starts it (--outdir DIR --step STEP): every step leaves a marker, "fail" exits with 3, "sleep" sleeps
TOOL = """import os, sys, time
outdir, step = (sys.argv[sys.argv.index(flag) + 1] for flag in ("--outdir", "--step"))
open(os.path.join(outdir, step + ".marker"), "w").close()
if step == "fail":
    sys.exit(3)
if step == "sleep":
    time.sleep(30)
"""
# rocprofv3's stand-in: records its arguments and its parent's command line, then runs what follows "--"
STUB = """#!/bin/sh
printf '%s\\n' "$@" > "$STUB_ARGV"
tr '\\0' '\\n' < /proc/$PPID/cmdline > "$STUB_PARENT"
while [ "$1" != "--" ]; do shift; done
shift
exec "$@"
"""


@pytest.fixture
def tool(tmp_path):
    path = tmp_path / "throwaway_time.py"
    path.write_text(TOOL)
    return str(path)


def run(tool, order, outdir, limit=20, **kw):
    """steps.run over ``order``; the message it exited with, or None if every step ended well"""
    try:
        steps.run(tool, dict.fromkeys(order), order, dict.fromkeys(order, limit), str(outdir), **kw)
    except SystemExit as e:
        assert e.code not in (None, 0)
        return str(e.code)
    return None


def test_a_failing_step_ends_the_chain(tool, tmp_path):
    message = run(tool, ("first", "fail", "third"), tmp_path)
    assert message == "[throwaway_time] step fail ended with status 3: nothing more is started on the GPU"
    assert (tmp_path / "first.marker").exists() and (tmp_path / "fail.marker").exists()
    assert not (tmp_path / "third.marker").exists()


def test_a_step_over_its_limit_ends_the_chain(tool, tmp_path):
    t0 = time.time()
    message = run(tool, ("sleep", "after"), tmp_path, limit=1)
    assert time.time() - t0 < 8
    assert "step sleep ended with status 124" in message
    assert (tmp_path / "sleep.marker").exists() and not (tmp_path / "after.marker").exists()


def test_every_step_runs_when_none_fails(tool, tmp_path):
    assert run(tool, ("first", "second"), tmp_path) is None
    assert (tmp_path / "first.marker").exists() and (tmp_path / "second.marker").exists()


def test_the_trace_step_runs_under_rocprofv3_inside_timeout(tool, tmp_path, monkeypatch):
    bindir = tmp_path / "bin"
    bindir.mkdir()
    stub = bindir / "rocprofv3"
    stub.write_text(STUB)
    stub.chmod(0o755)
    monkeypatch.setenv("PATH", f"{bindir}{os.pathsep}{os.environ['PATH']}")
    monkeypatch.setenv("STUB_ARGV", str(tmp_path / "argv"))
    monkeypatch.setenv("STUB_PARENT", str(tmp_path / "parent"))
    assert run(tool, ("first", "trace"), tmp_path, limit=7, trace_step="trace", trace_name="op") is None
    python = [sys.executable, tool, "--outdir", str(tmp_path), "--step", "trace"]
    rocprof = ["--kernel-trace", "--stats", "--output-format", "csv", "-d", str(tmp_path / "op_trace"), "-o", "op", "--"]
    assert (tmp_path / "argv").read_text().splitlines() == rocprof + python
    # timeout is outermost: it is the stub's parent, and the stub's own command line is what it was given to run
    assert (tmp_path / "parent").read_text().splitlines()[:4] == ["timeout", "-k", "10", "7"]
    assert (tmp_path / "trace.marker").exists()         # the program after "--" ran


@pytest.mark.parametrize("name", TOOLS)
def test_the_orchestrator_stays_off_the_gpu(name):
    """Loading a tool, as the orchestrating process does, imports no torch: only a ``--step`` child does."""
    code = ("import importlib.util, sys\n"
            f"spec = importlib.util.spec_from_file_location('tool', {os.path.join(ROOT, 'tools', name + '.py')!r})\n"
            "tool = importlib.util.module_from_spec(spec)\n"
            "spec.loader.exec_module(tool)\n"
            "assert callable(tool.finish) and all(map(callable, tool.STEPS.values())), 'no tool was loaded'\n"
            "sys.exit('torch was imported' if 'torch' in sys.modules else 0)\n")
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert done.returncode == 0, done.stderr


KERNELS = [("void k_fape_forward(float const*, int)", 20, 3540000.0), ("k_fape_backward(float const*, int)", 20, 26600000.0),
           ("at::native::vectorized_elementwise_kernel<4>(int)", 7, 1234.0)]
SPELLINGS = {"Name,Calls,TotalDurationNs,AverageNs,Percentage": lambda n, c, t: [n, c, t, t / c, 50.0],
             "name,total_calls,total_duration,average,percentage": lambda n, c, t: [n, c, t, t / c, 50.0]}


@pytest.mark.parametrize("header", SPELLINGS)
def test_kernel_stats_finds_the_csv_in_either_spelling(header, tmp_path):
    import csv
    (tmp_path / "host" / "1234").mkdir(parents=True)
    with open(tmp_path / "host" / "1234" / "op_kernel_stats.csv", "w", newline="") as f:
        csv.writer(f).writerows([header.split(",")] + [SPELLINGS[header](*k) for k in KERNELS])
    rows = steps.kernel_stats(str(tmp_path))
    assert rows[0] == header.lower().split(",")
    assert rows[1:] == [[n, str(c), str(t), str(t / c), "50.0"] for n, c, t in KERNELS]     # the same for both spellings
    assert fape_time.kernel_trace_times(str(tmp_path)) == {
        "k_fape_forward": {"calls": 20, "average_us": 3540000.0 / 20 / 1e3},
        "k_fape_backward": {"calls": 20, "average_us": 26600000.0 / 20 / 1e3}}


def test_kernel_stats_without_a_csv(tmp_path):
    assert steps.kernel_stats(str(tmp_path)) == []
    assert fape_time.kernel_trace_times(str(tmp_path)) == {}
    (tmp_path / "op_kernel_stats.csv").write_text("")       # what a rocprofv3 that was killed can leave
    assert steps.kernel_stats(str(tmp_path)) == []


def test_kernel_stats_joins_the_files_of_several_traced_processes(tmp_path):
    for pid, kernel in (("1", "k_a(int)"), ("2", "k_b(int)")):
        (tmp_path / pid).mkdir()
        (tmp_path / pid / "op_kernel_stats.csv").write_text(f"Name,Calls\n{kernel},3\n")
    assert steps.kernel_stats(str(tmp_path)) == [["name", "calls"], ["k_a(int)", "3"], ["k_b(int)", "3"]]


def test_largest_batch_drops_the_failed_attempt_before_emptying_the_cache(monkeypatch):
    """An attempt that ran out of memory must not keep its tensors (locals of ``measure``'s frame, which the exception's
    traceback holds) alive while the cache is emptied for the next, smaller one."""
    class Tensor:
        pass

    held, alive_at_empty_cache = [], []
    for name in ("synchronize", "reset_peak_memory_stats"):
        monkeypatch.setattr(torch.cuda, name, lambda: None)
    monkeypatch.setattr(torch.cuda, "empty_cache", lambda: alive_at_empty_cache.append([r() is not None for r in held]))
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda: 100)
    monkeypatch.setattr(torch.cuda, "max_memory_allocated", lambda: 350)

    def measure(b):
        x = Tensor()
        held.append(weakref.ref(x))
        if b > 2:
            raise torch.cuda.OutOfMemoryError(f"no room for a batch of {b}")
        return {"median_us": float(b)}

    assert steps.largest_batch_that_fits(8, measure) == {"batch": 2, "median_us": 2.0, "peak_bytes_allocated": 250,
                                                         "measured_at_full_batch": False}
    assert alive_at_empty_cache and not any(any(alive) for alive in alive_at_empty_cache)
    assert steps.largest_batch_that_fits(2, measure)["measured_at_full_batch"] is True
    assert steps.largest_batch_that_fits(1, lambda b: measure(3)) == {"batch": 0}


@pytest.mark.gpu
def test_timed_on_the_gpu():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    a, b = torch.ones(1024, device="cuda"), torch.ones(1024, device="cuda")
    t = steps.timed(lambda: torch.add(a, b), warmup=1, reps=5)
    assert set(t) == {"median_us", "min_us", "reps", "warmup"} and (t["reps"], t["warmup"]) == (5, 1)
    assert 0 < t["min_us"] <= t["median_us"]
