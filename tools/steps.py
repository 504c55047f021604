"""What an operator timing tool (tools/*_time.py) needs besides its own shapes and step bodies: the events timer, the
copy-rate probe, the largest-batch-that-fits loop of a composed-torch run, the reader of rocprofv3's kernel statistics,
and the step runner.

A tool is a dict of step functions ``step(outdir)``, a tuple with their order and a dict of time limits, handed to
``main``.  The orchestrating process never touches the GPU (no torch at module level, here or in a tool): every step is a
fresh child process of the tool's own file under its own ``timeout``, and the steps are chained -- the first one that
fails, faults or runs out of time ends the run, and nothing more is started on the card.
"""
import argparse
import csv
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(fn, warmup=3, reps=20):
    """HIP events around each call of ``fn``: median and minimum of ``reps`` after ``warmup`` calls, in microseconds."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return {"median_us": ts[len(ts) // 2], "min_us": ts[0], "reps": reps, "warmup": warmup}


def copy_rate():
    """bytes per second of a device-to-device copy of 1 GiB (read + write counted), and the copy's ``timed`` record"""
    import torch
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    t = timed(lambda: dst.copy_(src))
    return 2 * src.numel() * 4 / (t["median_us"] * 1e-6), t


def largest_batch_that_fits(B, measure):
    """``measure(b)``'s dict at the largest batch b = B, B / 2, ..., 1 at which it does not run out of GPU memory, with
    ``batch``, the allocator's peak over that call and ``measured_at_full_batch``; ``{"batch": 0}`` if none fits."""
    import torch
    b = B
    while b >= 1:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        try:
            return {"batch": b, **measure(b), "peak_bytes_allocated": torch.cuda.max_memory_allocated() - before,
                    "measured_at_full_batch": b == B}
        except torch.cuda.OutOfMemoryError:
            pass
        # only here, with the handler left, is the exception gone, and with its traceback measure's frame and the tensors
        # that frame held: inside the handler empty_cache would find them all still allocated
        torch.cuda.empty_cache()
        b //= 2
    return {"batch": 0}


def kernel_stats(tracedir):
    """rocprofv3's kernel_stats csv files, wherever under ``tracedir`` it wrote them (one per traced process): the header
    row, lower-cased, then every file's rows; no rows at all if there is no such file or none has a header."""
    out = []
    for path in sorted(glob.glob(os.path.join(tracedir, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path, newline="") as f:
            rows = list(csv.reader(f))
        if rows:
            out += rows[1:] if out else [[c.lower() for c in rows[0]]] + rows[1:]
    return out


def run(tool_file, steps, order, timeouts, outdir, trace_step=None, trace_name=None):
    """Run the steps of ``order`` one after the other, each as ``tool_file --outdir outdir --step STEP`` in a process of
    its own under ``timeout -k 10 timeouts[STEP]``, ``trace_step`` under ``rocprofv3 --kernel-trace --stats`` writing to
    ``outdir/<trace_name>_trace``.  The first step that ends with a non-zero status ends this process with a message."""
    tag = "[" + os.path.splitext(os.path.basename(tool_file))[0] + "]"
    assert set(order) <= set(steps) and set(order) <= set(timeouts), "every step needs a function and a time limit"
    for step in order:
        cmd = [sys.executable, os.path.abspath(tool_file), "--outdir", outdir, "--step", step]
        if step == trace_step:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d",
                   os.path.join(outdir, trace_name + "_trace"), "-o", trace_name, "--"] + cmd
        cmd = ["timeout", "-k", "10", str(timeouts[step])] + cmd
        print(tag, " ".join(cmd), flush=True)
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            sys.exit(f"{tag} step {step} ended with status {rc}: nothing more is started on the GPU")


def main(tool_file, steps, order, timeouts, finish, trace_step=None, trace_name=None, optional=()):
    """The tools' command line: ``[--outdir DIR] [--step STEP]`` and a ``--no-STEP`` flag for each step of ``optional``.
    With ``--step``, run that step here, on the GPU; without, run the steps of ``order`` as child processes and then
    ``finish(outdir)``, which merges what they wrote into the report."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--step", choices=sorted(steps))
    for step in optional:
        ap.add_argument("--no-" + step, action="store_true")
    args = ap.parse_args()
    outdir = os.path.abspath(args.outdir)      # the steps run from the repository root, wherever this was started
    os.makedirs(outdir, exist_ok=True)
    if args.step:
        import torch
        assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
        steps[args.step](outdir)
        return
    order = tuple(s for s in order if not getattr(args, "no_" + s, False))
    run(tool_file, steps, order, timeouts, outdir, trace_step, trace_name)
    finish(outdir)
