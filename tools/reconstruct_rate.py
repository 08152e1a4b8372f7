#!/usr/bin/env python3
"""Times, launch counts and working-tile shares of the geodesic operations on the device (vpt_volume_geodesic_timed) at 256^3 R8, the two
configurations of DESIGN.md "Geodesic reconstruction":

  sphere   fill_holes of a hollow sphere (radii 90 .. 100), under 6- and 26-connectivity; where scipy imports, the result is also held
           to scipy.ndimage.binary_fill_holes
  balls    300 random overlapping balls (radii 8 .. 20): distance 'rest' -> channel(steps=4) -> hmax(4) of channel 1 -> regional_maxima,
           under 26-connectivity; the structures and the seeds are counted with Volume.components

    python tools/reconstruct_rate.py [--out profiles/reconstruct_rates.json] [--step-timeout 300]

Each configuration runs in a child process of its own under its own time limit; the first that fails or runs out of time ends the run and
nothing further is started.  A figure is the median of 5 timed calls after a warm-up; the time is the library's own (the call up to the
result's finalize, the stream drained either side).  share = tiles that did LDS work / (launches x tiles of the volume)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 256
TILES = (N // 64) * (N // 8) * (N // 4)
RUNS = 6                                                          # a warm-up and five


def timed(call):
    """{'ms_median', 'ms_min', 'ms_max', 'launches', 'tile_runs', 'share'} of RUNS - 1 calls after a warm-up, and the last volume made"""
    profiles, last = [], None
    for _ in range(RUNS):
        if last is not None:
            last.destroy()
        last, p = call()
        profiles.append(p)
    ms = sorted(p['ms'] for p in profiles[1:])
    p = profiles[-1]
    return {'ms_median': ms[len(ms) // 2], 'ms_min': ms[0], 'ms_max': ms[-1], 'launches': p['launches'], 'tile_runs': p['tile_runs'],
            'share': p['tile_runs'] / (p['launches'] * TILES)}, last


def run_sphere():
    import vpt_amd
    z, y, x = np.mgrid[0:N, 0:N, 0:N].astype(np.float32)
    r = np.sqrt((x - 127.5) ** 2 + (y - 127.5) ** 2 + (z - 127.5) ** 2)
    a = np.where((r <= 100) & (r >= 90), 200, 0).astype(np.uint8)
    ctx = vpt_amd.Context(0)
    v = vpt_amd.Volume.from_array(ctx, a)
    row = {}
    for c in (6, 26):
        row['fill_holes %d' % c], out = timed(lambda: v.fill_holes_timed(c))
        got = out.read_block(0, 0, 0, N, N, N)
        out.destroy()
        row['fill_holes %d' % c]['filled_voxels'] = int(np.count_nonzero(got != a))
        try:
            from scipy import ndimage
            want = ndimage.binary_fill_holes(a > 0, structure=ndimage.generate_binary_structure(3, 1 if c == 6 else 3))
            row['fill_holes %d' % c]['equals_scipy'] = bool(((got > 0) == want).all())
        except ImportError:
            pass
    v.destroy(); ctx.destroy()
    return row


def run_balls():
    import vpt_amd
    rng = np.random.default_rng(5)
    a = np.zeros((N, N, N), np.uint8)
    for _ in range(300):
        rad = int(rng.integers(8, 21))
        c = rng.integers(rad, N - rad, size=3)
        zz, yy, xx = np.mgrid[-rad:rad + 1, -rad:rad + 1, -rad:rad + 1]
        a[c[0] - rad:c[0] + rad + 1, c[1] - rad:c[1] + rad + 1, c[2] - rad:c[2] + rad + 1][zz * zz + yy * yy + xx * xx <= rad * rad] = 200
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, a)
    found = src.components(100, 255, 26)
    row = {'foreground': float((a > 0).mean()), 'structures': found.info['listed']}
    found.destroy()
    d = src.distance(100, 255, 'rest')
    depth = d.channel(steps=4)
    d.destroy()
    row['hmax 4'], flattened = timed(lambda: depth.hmax_timed(4, 26, channel=1))
    row['regional_maxima'], maxima = timed(lambda: flattened.regional_maxima_timed(26))
    found = maxima.components(255, 255, 26)
    row['seeds'] = found.info['listed']
    found.destroy()
    for vol in (maxima, flattened, depth, src):
        vol.destroy()
    ctx.destroy()
    return row


def child(step, limit):
    """the JSON a child process of this script prints last, or None when it failed or ran out of time"""
    try:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], stdout=subprocess.PIPE, timeout=limit)
    except subprocess.TimeoutExpired:
        print("step %r ran out of its %d s" % (step, limit), file=sys.stderr)
        return None
    if res.returncode != 0:
        print("step %r ended with %d" % (step, res.returncode), file=sys.stderr)
        return None
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--step", default=None, help="(internal) 'sphere' or 'balls'")
    a = ap.parse_args()
    if a.step is not None:
        print(json.dumps(run_sphere() if a.step == "sphere" else run_balls()))
        return 0
    out = {"volume": "256^3 R8", "tiles": TILES,
           "timing": "the library's own time of the call up to the result's finalize, stream drained either side; median of 5 after a warm-up; clocks not pinned",
           "not_measured": ["R16", "volumes beyond 256^3", "the Node.js host", "hardware counters", "per-launch shares (the share is the mean over a call's launches)"]}
    for step in ("sphere", "balls"):
        row = child(step, a.step_timeout)
        if row is None:
            return 1
        out[step] = row
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
