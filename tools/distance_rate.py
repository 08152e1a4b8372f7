#!/usr/bin/env python3
"""Times of the distance transform on the device (vpt_volume_distance and the within / channel emitters), per phase and per whole call,
for R8 volumes of three kinds: (a) the synthetic sphere volume, the range its shell (codes 40 .. 120), (b) one seed in a corner (the
longest parabolas, every lane's stack of depth 1), (c) uniform noise at density 0.30.  Each with the seeds in the range (TO_RANGE) and
outside it (TO_REST).  Beside them the yardsticks taken in the same run: the device's streaming-read rate (vpt_probe_stream_read) and the
wall time of scipy.ndimage.distance_transform_edt on the same array on this machine's CPUs (where scipy is installed).

    python tools/distance_rate.py [--out profiles/distance_rates.json] [--sizes 256 512] [--step-timeout 300]

Every step that uses the device (the probe, and each case at each size) runs in a child process of its own under its own time limit; the
first step that fails or runs out of time ends the run and nothing further is started.

The phase times are the library's own (vpt_distance_profile: wall time of each pass, the stream drained at its end), those of the
shortest whole call of 3 after a warm-up; within and channel are whole calls (allocation, kernel, finalize of the result).  A pass streams
at least 4 B in and 4 B out per voxel (x: the texel in, so 1 + 4) beside its stack: the rates below are these bytes over the pass's time."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_VOXEL = {"x": 5, "y": 8, "z": 8, "within": 6, "channel": 7}       # R8
CASES = ("sphere shell", "corner seed", "noise 0.30")


def case_volume(name, n):
    """(uint8 [n][n][n], lo, hi)"""
    if name == "sphere shell":
        from vpt_amd.synthetic import sphere_volume
        return sphere_volume(n, noise=48.0), 40, 120
    if name == "corner seed":
        a = np.zeros((n, n, n), np.uint8)
        a[0, 0, 0] = 200
        return a, 200, 200
    return np.random.default_rng(n).integers(0, 256, size=(n, n, n)).astype(np.uint8), 0, 76


def host_transform(a, lo, hi, seeds):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    seed = ((a >= lo) & (a <= hi)) != (seeds == 'rest')
    t0 = time.perf_counter()
    d = ndimage.distance_transform_edt(~seed)
    return {"what": "scipy.ndimage.distance_transform_edt", "ms": (time.perf_counter() - t0) * 1e3, "largest": int(round(float(d.max()) ** 2))}


def run_probe():
    import vpt_amd
    ctx = vpt_amd.Context(0)
    rate = ctx.stream_read_rate(1 << 30, 5)
    ctx.destroy()
    return {"stream_read_GB_per_s": rate}


def run_case(name, n, probe, host):
    import vpt_amd
    vol, lo, hi = case_volume(name, n)
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, vol)
    voxels = float(n) ** 3
    out = {}
    for seeds in ('range', 'rest'):
        best, found = None, None
        for run in range(4):
            ctx.synchronize()
            t0 = time.perf_counter()
            found = src.distance(lo, hi, seeds)
            whole = time.perf_counter() - t0
            if run and (best is None or whole < best[0]):
                best = (whole, found.profile(), found.info)
            if run < 3:
                found.destroy()
        whole, phases, info = best
        row = {"whole_call_ms": whole * 1e3, "phases_ms": phases, "info": info}
        for emitter, call in (("within", lambda: found.within(0, 9)), ("channel", lambda: found.channel(4))):
            times = []
            for _ in range(4):
                ctx.synchronize()
                t0 = time.perf_counter()
                v = call()
                ctx.synchronize()
                times.append(time.perf_counter() - t0)
                v.destroy()
            row[emitter + "_call_ms"] = min(times[1:]) * 1e3
        found.destroy()
        for phase in ("x", "y", "z"):
            rate = BYTES_PER_VOXEL[phase] * voxels / (phases[phase] * 1e-3) / 1e9
            row[phase + "_GB_per_s"] = rate
            row[phase + "_fraction_of_stream_read"] = rate / probe
        for emitter in ("within", "channel"):
            rate = BYTES_PER_VOXEL[emitter] * voxels / (row[emitter + "_call_ms"] * 1e-3) / 1e9
            row[emitter + "_call_GB_per_s"] = rate
            row[emitter + "_call_fraction_of_stream_read"] = rate / probe
        if host:
            row["host"] = host_transform(vol, lo, hi, seeds)
        out[seeds] = row
    src.destroy()
    ctx.destroy()
    return out


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
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--no-host", action="store_true", help="skip the host transform")
    ap.add_argument("--step", nargs="+", default=None, help="(internal) 'probe', or a case's name, its size and the probe's rate")
    a = ap.parse_args()
    if a.step is not None:
        row = run_probe() if a.step[0] == "probe" else run_case(a.step[0], int(a.step[1]), float(a.step[2]), not a.no_host)
        print(json.dumps(row))
        return 0
    probe = child(["--step", "probe"], a.step_timeout)
    if probe is None:
        return 1
    out = dict(probe, bytes_per_voxel=BYTES_PER_VOXEL, cases={}, corner_over_noise={})
    failed = False
    for n in a.sizes:
        for name in CASES:
            row = child(["--step", name, str(n), repr(probe["stream_read_GB_per_s"])] + (["--no-host"] if a.no_host else []), a.step_timeout)
            if row is None:
                failed = True
                break
            out["cases"]["%d^3 %s" % (n, name)] = row
            print("%d^3 %s: TO_RANGE %.2f ms, TO_REST %.2f ms" % (n, name, row["range"]["whole_call_ms"], row["rest"]["whole_call_ms"]), file=sys.stderr, flush=True)
        if failed:
            break
        # a design whose time on the corner seed grows with the distance rather than with the voxel count shows up here
        corner, dense = out["cases"]["%d^3 corner seed" % n]["range"], out["cases"]["%d^3 noise 0.30" % n]["range"]
        out["corner_over_noise"]["%d^3" % n] = dict({p: corner["phases_ms"][p] / dense["phases_ms"][p] for p in ("x", "y", "z")},
                                                    whole_call=corner["whole_call_ms"] / dense["whole_call_ms"])
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
