#!/usr/bin/env python3
"""Times of the resampling on the device (vpt_volume_resample), per whole call and per pass, for R8 and R16 volumes of uniform noise:

    512 x 512 x 200 -> 512 x 512 x 571   the isotropic grid of a CT with 0.7 x 0.7 x 2.0 mm voxels: one axis grows
    512^3 -> 256^3                       beside Volume.reduce() of the same volume in the same run: the same arithmetic, the ratio is the
                                         price of generality
    512^3 -> 300^3                       a non-integer shrink
    256^3 -> 512^3                       a doubling
    512^3 -> 300^3, NEAREST

Beside them the yardsticks taken in the same run: the device's streaming-read rate (vpt_probe_stream_read) and the wall time of
scipy.ndimage.zoom(order=1) on the same array on this machine's CPUs where scipy is installed (for scale only: its alignment and rounding
differ from the contract).

    python tools/resample_rate.py [--out profiles/resample_rates.json] [--step-timeout 300] [--no-host]

Every step that uses the device (the probe, and each case in each format) runs in a child process of its own under its own time limit; the
first step that fails or runs out of time ends the run and nothing further is started.

The whole call is the shortest of 3 after a warm-up, the finalize of the result (brick layout, boundary atlas) included and the stream
drained at its end.  The passes are the library's own times (vpt_volume_resample_timed: wall time of each pass, the stream drained after
it), those of the shortest of 3 timed calls after a warm-up.  Bytes counted, B = bytes per texel, P = the partial sums' texels (result
width x source height x source depth): row pass source B + 4 P, plane pass 4 P + result B (every partial sum counted once, although
neighbouring result rows and planes share taps), NEAREST 2 x result B."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (source (depth, height, width), target (depth, height, width), mode, also time reduce())
CASES = {
    "CT 512x512x200 -> isotropic 512x512x571": ((200, 512, 512), (571, 512, 512), 'filtered', False),
    "512^3 -> 256^3": ((512, 512, 512), (256, 256, 256), 'filtered', True),
    "512^3 -> 300^3": ((512, 512, 512), (300, 300, 300), 'filtered', False),
    "256^3 -> 512^3": ((256, 256, 256), (512, 512, 512), 'filtered', False),
    "512^3 -> 300^3 nearest": ((512, 512, 512), (300, 300, 300), 'nearest', False),
}
FORMATS = {"R8": np.uint8, "R16": np.uint16}


def host_zoom(a, target):
    try:
        from scipy import ndimage
    except ImportError:
        return {"what": "scipy.ndimage.zoom(order=1)", "available": False}
    t0 = time.perf_counter()
    out = ndimage.zoom(a, [t / s for t, s in zip(target, a.shape)], order=1)
    return {"what": "scipy.ndimage.zoom(order=1)", "available": True, "ms": (time.perf_counter() - t0) * 1e3, "shape": list(out.shape)}


def run_probe():
    import vpt_amd
    ctx = vpt_amd.Context(0)
    rate = ctx.stream_read_rate(1 << 30, 5)
    ctx.destroy()
    return {"stream_read_GB_per_s": rate}


def shortest(ctx, call, runs=4):
    """milliseconds of the shortest of runs - 1 calls after a warm-up, the stream drained around each; what the last call returned"""
    times, out = [], None
    for run in range(runs):
        if out is not None:
            (out[0] if isinstance(out, tuple) else out).destroy()
        ctx.synchronize()
        t0 = time.perf_counter()
        out = call()
        ctx.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times[1:]), out


def run_case(name, fmt, probe, host):
    import vpt_amd
    source, target, mode, with_reduce = CASES[name]
    dtype = FORMATS[fmt]
    a = np.random.default_rng(len(name)).integers(0, int(np.iinfo(dtype).max) + 1, size=source).astype(dtype)
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, a, norm16=dtype == np.uint16)
    d, h, w = target
    B = a.dtype.itemsize
    row = {"source": list(source), "target": list(target), "mode": mode, "format": fmt}
    row["whole_call_ms"], out = shortest(ctx, lambda: src.resample(w, h, d, mode))
    out.destroy()
    result_bytes = float(d) * h * w * B
    if mode == 'filtered':
        best = None
        for run in range(4):
            vol, ms = src.resample_timed(w, h, d, mode)
            vol.destroy()
            if run and (best is None or ms['x'] + ms['yz'] < best['x'] + best['yz']):
                best = ms
        partial = float(w) * source[1] * source[0]
        moved = {"x": a.nbytes + 4 * partial, "yz": 4 * partial + result_bytes}
        row["passes_ms"], row["bytes_counted"] = best, moved
        for phase in ("x", "yz"):
            rate = moved[phase] / (best[phase] * 1e-3) / 1e9
            row[phase + "_GB_per_s"] = rate
            row[phase + "_fraction_of_stream_read"] = rate / probe
    else:
        moved = 2 * result_bytes
        rate = moved / (row["whole_call_ms"] * 1e-3) / 1e9
        row["bytes_counted"] = {"whole_call": moved}
        row["whole_call_GB_per_s"], row["whole_call_fraction_of_stream_read"] = rate, rate / probe
    if with_reduce:
        row["reduce_whole_call_ms"], out = shortest(ctx, lambda: src.reduce())
        out.destroy()
        row["resample_over_reduce"] = row["whole_call_ms"] / row["reduce_whole_call_ms"]
    src.destroy()
    ctx.destroy()
    if host:
        row["host"] = host_zoom(a, target)
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
    ap.add_argument("--no-host", action="store_true", help="skip scipy.ndimage.zoom")
    ap.add_argument("--step", nargs="+", default=None, help="(internal) 'probe', or a case's name, its format and the probe's rate")
    a = ap.parse_args()
    if a.step is not None:
        row = run_probe() if a.step[0] == "probe" else run_case(a.step[0], a.step[1], float(a.step[2]), not a.no_host)
        print(json.dumps(row))
        return 0
    probe = child(["--step", "probe"], a.step_timeout)
    if probe is None:
        return 1
    out = dict(probe, timing="whole call: shortest of 3 after a warm-up, finalize included, stream drained; passes: stream drained after each",
               not_measured=["two-channel formats (RG8, RG16)", "volumes beyond 512^3", "the Node.js host", "more than one device"], cases={})
    failed = False
    for name in CASES:
        for fmt in FORMATS:
            row = child(["--step", name, fmt, repr(probe["stream_read_GB_per_s"])] + (["--no-host"] if a.no_host else []), a.step_timeout)
            if row is None:
                failed = True
                break
            out["cases"]["%s %s" % (fmt, name)] = row
            print("%s %s: %.2f ms" % (fmt, name, row["whole_call_ms"]), file=sys.stderr, flush=True)
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
