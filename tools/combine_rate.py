#!/usr/bin/env python3
"""Times of the two-volume operations on the device (vpt_volume_combine, vpt_volume_compare) for R8 and R16 volumes of uniform noise at
256^3 and 512^3: the ops MASK, BLEND and PAIR, and compare.  Each as a whole call (the finalize of the result included) and as the
combining pass alone (vpt_volume_combine_timed), and each expressed as a fraction of the device's streaming-read rate
(vpt_probe_stream_read over 1 GiB, taken in the same run) at the algorithmic bytes per voxel: B(a) + B(b) + B(result), compare B(a) + B(b).
Beside them Distance.within of the same volume: k_select, the sibling of the same streaming form (texel + one uint32 in, texel out).

    python tools/combine_rate.py [--out profiles/combine_rates.json] [--step-timeout 300]

Every step that uses the device (the probe, and each size in each format) runs in a child process of its own under its own time limit; the
first step that fails or runs out of time ends the run and nothing further is started.

The whole call is the shortest of 5 after a warm-up, the stream drained at its end.  The pass is the library's own time (wall time of the
launch with the stream drained in front of it and behind it, so it carries the launch and the synchronisation, tens of microseconds), the
shortest of 5 timed calls after a warm-up."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"256^3": 256, "512^3": 512}
FORMATS = {"R8": np.uint8, "R16": np.uint16}
RUNS = 6                                                          # a warm-up and five


def run_probe():
    import vpt_amd
    ctx = vpt_amd.Context(0)
    rate = ctx.stream_read_rate(1 << 30, 5)
    ctx.destroy()
    return {"stream_read_GB_per_s": rate}


def shortest(ctx, call):
    """milliseconds of the shortest of RUNS - 1 calls after a warm-up, the stream drained around each; a returned volume is destroyed"""
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


def run_case(size, fmt, probe):
    import vpt_amd
    n, dtype = SIZES[size], FORMATS[fmt]
    rng = np.random.default_rng(n)
    M = int(np.iinfo(dtype).max)
    a = rng.integers(0, M + 1, size=(n, n, n)).astype(dtype)
    b = rng.integers(0, M + 1, size=(n, n, n)).astype(dtype)
    ctx = vpt_amd.Context(0)
    va, vb = vpt_amd.Volume.from_array(ctx, a, norm16=dtype == np.uint16), vpt_amd.Volume.from_array(ctx, b, norm16=dtype == np.uint16)
    B, voxels = a.dtype.itemsize, float(a.size)
    row = {"size": size, "format": fmt, "ops": {}}
    ops = {"mask": ({'lo': M // 4, 'hi': M}, 3 * B), "blend": ({'wa': 160, 'wb': 96, 'offset': 0}, 3 * B), "pair": ({}, 4 * B)}
    for op, (params, per_voxel) in ops.items():
        whole = shortest(ctx, lambda: va.combine(vb, op, **params))
        passes = []
        for _ in range(RUNS):
            vol, ms = va.combine_timed(vb, op, **params)
            vol.destroy()
            passes.append(ms)
        kernel = min(passes[1:])
        rate = per_voxel * voxels / (kernel * 1e-3) / 1e9
        row["ops"][op] = {"whole_call_ms": whole, "pass_ms": kernel, "bytes_per_voxel": per_voxel, "pass_GB_per_s": rate, "pass_fraction_of_stream_read": rate / probe}
    whole = shortest(ctx, lambda: va.compare(vb, (M // 4, M), (M // 2, M)))
    rate = 2 * B * voxels / (whole * 1e-3) / 1e9
    row["ops"]["compare"] = {"whole_call_ms": whole, "bytes_per_voxel": 2 * B, "whole_call_GB_per_s": rate, "whole_call_fraction_of_stream_read": rate / probe}
    found = va.distance(M // 2, M)                                # the sibling: k_select over the texels and one uint32 a voxel
    whole = shortest(ctx, lambda: found.within(0, 4))
    found.destroy()
    row["distance_within"] = {"whole_call_ms": whole, "bytes_per_voxel": 2 * B + 4, "note": "whole call only: the emitter has no timed form"}
    va.destroy(); vb.destroy()
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
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--step", nargs="+", default=None, help="(internal) 'probe', or a size, a format and the probe's rate")
    a = ap.parse_args()
    if a.step is not None:
        row = run_probe() if a.step[0] == "probe" else run_case(a.step[0], a.step[1], float(a.step[2]))
        print(json.dumps(row))
        return 0
    probe = child(["--step", "probe"], a.step_timeout)
    if probe is None:
        return 1
    out = dict(probe, timing="whole call: shortest of 5 after a warm-up, finalize included, stream drained; pass: the launch alone, stream drained around it",
               not_measured=["two-channel second volumes", "mixed widths", "volumes beyond 512^3", "the Node.js host", "hardware counters"], cases={})
    failed = False
    for size in SIZES:
        for fmt in FORMATS:
            row = child(["--step", size, fmt, repr(probe["stream_read_GB_per_s"])], a.step_timeout)
            if row is None:
                failed = True
                break
            out["cases"]["%s %s" % (fmt, size)] = row
            print("%s %s: blend pass %.3f ms" % (fmt, size, row["ops"]["blend"]["pass_ms"]), file=sys.stderr, flush=True)
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
