#!/usr/bin/env python3
"""Times of the per-component measuring pass on the device (vpt_components_measure_timed) at 512^3, R8 and R16, for three contents:

    ball          a filled ball: one giant component, every workgroup adds to one record
    noise         6-connected noise at a foreground fraction of 0.30: many small components
    checkerboard  (x + y + z) even under 6-connectivity: one record per foreground voxel, the worst case for the workgroup's table

Each is set against the bytes the pass must read, the ranks (4 a voxel) and the values (1 or 2 a voxel), at the streaming-read rate that
profiles/combine_rates.json records for this chip.  Beside them the whole call of keep_set (half of the list, a prepared rank array) and of
keep over the same ranks, ball and noise only.

    python tools/measure_rate.py [--out profiles/measure_rates.json] [--step-timeout 600]

Every content in each format runs in a child process of its own under its own time limit; the first step that fails or runs out of time
ends the run and nothing further is started.  The pass is the library's own time (wall time of the launch with the stream drained in front
of it and behind it), the shortest of 4 timed calls after a warm-up; the whole calls are the shortest of 4 after a warm-up, the stream
drained at their end."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE = 512
FORMATS = {"R8": np.uint8, "R16": np.uint16}
CONTENTS = ("ball", "noise", "checkerboard")
RUNS = 5                                                          # a warm-up and four


def content(name, dtype):
    """(texels, lo, hi) of a SIZE^3 volume"""
    n, M = SIZE, int(np.iinfo(dtype).max)
    if name == "noise":
        a = np.random.default_rng(n).integers(0, M + 1, size=(n, n, n)).astype(dtype)
        return a, 0, int(round(0.30 * (M + 1))) - 1
    z, y, x = np.ogrid[0:n, 0:n, 0:n]
    if name == "ball":
        inside = (x - n // 2) ** 2 + (y - n // 2) ** 2 + (z - n // 2) ** 2 <= (n * 3 // 8) ** 2
    else:
        inside = (x + y + z) % 2 == 0
    values = np.random.default_rng(n + 1).integers(M // 2, M + 1, size=(n, n, n)).astype(dtype)
    return np.where(inside, values, 0).astype(dtype), M // 2, M


def shortest(ctx, call):
    times = []
    for _ in range(RUNS):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = call()
        ctx.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        if hasattr(out, 'destroy'):
            out.destroy()
    return min(times[1:])


def run_case(name, fmt, stream_read):
    import vpt_amd
    from vpt_amd import _native as N
    dtype = FORMATS[fmt]
    a, lo, hi = content(name, dtype)
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, a, norm16=dtype == np.uint16)
    found = src.components(lo, hi, 6)
    src.destroy()
    listed = found.info['listed']
    out = np.zeros(listed, vpt_amd.MEASURE_DTYPE)
    dst, ms = out.ctypes.data_as(C.POINTER(N.ComponentMeasure)), C.c_double(0)
    passes = []
    for _ in range(RUNS):
        N.check(N.lib().vpt_components_measure_timed(found._h, None, 0, 0, listed, dst, C.byref(ms)))
        passes.append(ms.value)
    kernel = min(passes[1:])
    assert int(out['voxels'].sum()) == found.info['listed_voxels']
    per_voxel = 4 + a.dtype.itemsize
    rate = per_voxel * float(a.size) / (kernel * 1e-3) / 1e9
    row = {"content": name, "format": fmt, "size": "%d^3" % SIZE, "listed": listed, "listed_voxels": found.info['listed_voxels'], "pass_ms": kernel,
           "bytes_per_voxel": per_voxel, "pass_GB_per_s": rate, "pass_fraction_of_stream_read": rate / stream_read,
           "largest_component_faces": int(out['faces'][0])}
    if name != "checkerboard":
        k = max(listed // 2, 1)
        kept = np.arange(1, k + 1, dtype=np.uint64)
        ranks = kept.ctypes.data_as(C.POINTER(C.c_uint64))

        def keep_set():
            h = C.c_void_p()
            N.check(N.lib().vpt_components_keep_set(found._h, ranks, k, 0, C.byref(h)))
            return found._derived(h)

        row["keep_set_whole_call_ms"] = shortest(ctx, keep_set)
        row["keep_whole_call_ms"] = shortest(ctx, lambda: found.keep(1, k))
        row["kept_ranks"] = k
    found.destroy()
    ctx.destroy()
    return row


def child(args, limit):
    """the JSON a child process of this script prints last, or None when it failed or ran out of time"""
    try:
        res = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, timeout=limit)
    except subprocess.TimeoutExpired:
        print("step %r ran out of its %d s" % (args, limit), file=sys.stderr)
        return None
    if res.returncode != 0:
        print("step %r ended with %d" % (args, res.returncode), file=sys.stderr)
        return None
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--step", nargs="+", default=None, help="(internal) a content, a format and the streaming-read rate")
    a = ap.parse_args()
    if a.step is not None:
        print(json.dumps(run_case(a.step[0], a.step[1], float(a.step[2]))))
        return 0
    with open(os.path.join(ROOT, "profiles", "combine_rates.json")) as f:
        stream_read = json.load(f)["stream_read_GB_per_s"]
    out = {"stream_read_GB_per_s": stream_read, "stream_read_from": "profiles/combine_rates.json",
           "timing": "pass: the measuring launch alone, stream drained around it, shortest of 4 after a warm-up; whole calls: shortest of 4 after a warm-up, finalize included",
           "not_measured": ["values of another volume or width", "windows shorter than the list", "volumes beyond 512^3", "the Node.js host", "hardware counters"],
           "cases": {}}
    failed = False
    for fmt in FORMATS:
        for name in CONTENTS:
            row = child(["--step", name, fmt, repr(stream_read)], a.step_timeout)
            if row is None:
                failed = True
                break
            out["cases"]["%s %s" % (fmt, name)] = row
            print("%s %s: pass %.3f ms, %.3f of the streaming-read rate" % (fmt, name, row["pass_ms"], row["pass_fraction_of_stream_read"]), file=sys.stderr, flush=True)
        if failed:
            break
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
