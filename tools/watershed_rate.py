#!/usr/bin/env python3
"""Times and launch counts of the watershed on the device at 256^3 R8, the workload of DESIGN.md "Geodesic reconstruction" carried to its
end: 300 random overlapping balls (radii 8 .. 20), distance 'rest' -> channel(steps=4) -> hmax(2) of channel 1 -> watershed(1, 255, 'maxima')
under 26-connectivity with the balls as texels: what ``Volume.split(100, 255)`` runs.  Three configurations:

  watershed   the watershed step of the split: its three phases (vpt_volume_watershed_timed), the common tail (vpt_components_profile),
              the plateau, merge and flatten launch counts, the basins
  components  vpt_volume_components of the same foreground (the codes 100 .. 255 of the balls) under 26-connectivity, per phase
  maxima      regional_maxima of the same channel (the flattened depth) under 26-connectivity

    python tools/watershed_rate.py [--out profiles/watershed_rates.json] [--step-timeout 300] [--parent-tree PATH]

--parent-tree: a built checkout of the parent commit; 'components' and 'maxima' then import vpt_amd (and its library) from there, so that
the comparison is with the code as it stood before the watershed.

Each configuration runs in a child process of its own under its own time limit; the first that fails or runs out of time ends the run and
nothing further is started.  A figure is the median of 5 timed calls after a warm-up; the times are the library's own (a phase up to the
drained stream)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 256
RUNS = 6                                                          # a warm-up and five
TAIL = ('tiles', 'merge', 'flatten', 'sizes', 'compaction', 'sort', 'ranks')


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def balls():
    rng = np.random.default_rng(5)
    a = np.zeros((N, N, N), np.uint8)
    for _ in range(300):
        rad = int(rng.integers(8, 21))
        c = rng.integers(rad, N - rad, size=3)
        zz, yy, xx = np.mgrid[-rad:rad + 1, -rad:rad + 1, -rad:rad + 1]
        a[c[0] - rad:c[0] + rad + 1, c[1] - rad:c[1] + rad + 1, c[2] - rad:c[2] + rad + 1][zz * zz + yy * yy + xx * xx <= rad * rad] = 200
    return a


def flattened_depth(src):
    d = src.distance(100, 255, 'rest')
    depth = d.channel(steps=4)
    d.destroy()
    flattened = depth.hmax(2, 26, channel=1)
    depth.destroy()
    return flattened


def phases(profiles, names):
    return {name: median(p[name] for p in profiles) for name in names}


def run_watershed():
    import vpt_amd
    a = balls()
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, a)
    flattened = flattened_depth(src)
    own, tail, row = [], [], {}
    for _ in range(RUNS):
        basins, profile = flattened.watershed_timed(1, 255, 'maxima', 26, texels=src)
        ms, merges, flattens = basins.profile()
        own.append(profile['ms']); tail.append(ms)
        row.update(plateau_launches=profile['plateau_launches'], merge_launches=merges, flatten_launches=flattens, basins=basins.info['listed'],
                   domain_voxels=basins.info['foreground_voxels'])
        basins.destroy()
    row['ms'] = phases(own[1:], ('classify', 'plateau', 'links'))
    row['ms_tail'] = phases(tail[1:], TAIL[1:])                   # 'tiles' is the three phases above together
    row['ms_total'] = median(sum(o.values()) + sum(t[name] for name in TAIL[1:]) for o, t in zip(own[1:], tail[1:]))
    flattened.destroy(); src.destroy(); ctx.destroy()
    return row


def run_components():
    import vpt_amd
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, balls())
    profiles, row = [], {}
    for _ in range(RUNS):
        found = src.components(100, 255, 26)
        ms, merges, flattens = found.profile()
        profiles.append(ms)
        row.update(merge_launches=merges, flatten_launches=flattens, structures=found.info['listed'], foreground_voxels=found.info['foreground_voxels'])
        found.destroy()
    row['ms'] = phases(profiles[1:], TAIL)
    row['ms_total'] = median(sum(p.values()) for p in profiles[1:])
    src.destroy(); ctx.destroy()
    return row


def run_maxima():
    import vpt_amd
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, balls())
    flattened = flattened_depth(src)
    profiles = []
    for _ in range(RUNS):
        out, p = flattened.regional_maxima_timed(26)
        out.destroy()
        profiles.append(p)
    row = {'ms_total': median(p['ms'] for p in profiles[1:]), 'launches': profiles[-1]['launches'], 'tile_runs': profiles[-1]['tile_runs']}
    flattened.destroy(); src.destroy(); ctx.destroy()
    return row


STEPS = {'watershed': run_watershed, 'components': run_components, 'maxima': run_maxima}


def child(step, limit, tree):
    """the JSON a child process of this script prints last, or None when it failed or ran out of time"""
    try:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + (["--parent-tree", os.path.abspath(tree)] if tree else []),
                             stdout=subprocess.PIPE, timeout=limit)
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
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit for 'components' and 'maxima'")
    ap.add_argument("--step", default=None, help="(internal) one of %s" % ", ".join(STEPS))
    a = ap.parse_args()
    if a.step is not None:
        if a.parent_tree:
            sys.path.insert(0, a.parent_tree)                     # in front of this tree: vpt_amd is the parent's
        print(json.dumps(STEPS[a.step]()))
        return 0
    out = {"volume": "256^3 R8, 300 random balls of radii 8 .. 20 (seed 5); the relief is hmax(2) of the depth channel (steps 4), 26-connectivity",
           "timing": "the library's own phase times, the stream drained at the end of each phase; median of 5 after a warm-up; a fresh process per "
                     "configuration; clocks not pinned.  ms_total is the sum of the phases: device allocations and frees (the watershed's d, flags "
                     "and direction codes; the count array and control words of both) lie between the phases and are in neither total",
           "components_and_maxima_tree": "the parent commit's" if a.parent_tree else "this tree's",
           "not_measured": ["R16", "volumes beyond 256^3", "the Node.js host", "hardware counters", "the distance, channel and hmax steps of split"]}
    for step in STEPS:
        row = child(step, a.step_timeout, a.parent_tree if step != 'watershed' else "")
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
