#!/usr/bin/env python3
"""Times and visit counts of local thickness on the device at 256^3 R8 (DESIGN.md "Local thickness"), two workloads:

  thin    the project's 300 random overlapping balls (radii 8 .. 20): many small structures
  thick   one ball of radius 100: one structure that crosses thousands of tiles

For each: the three phases of vpt_distance_thickness_timed (tile maxima and their ordering, the cover, info) of the distances to the rest
of the codes 100 .. 255, the listed tiles, the centre tiles a workgroup ran over per listed tile with both culls and (one run) with the value
cull switched off; and beside them, as the scale to read the figures against, the three phases of vpt_volume_distance on the same input.

    python tools/thickness_rate.py [--out profiles/thickness_rates.json] [--step-timeout 300] [--parent-tree PATH]

--parent-tree: a built checkout of the parent commit; the distance rows then import vpt_amd (and its library) from there, so that the scale
is the code as it stood before this unit.

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


def median(values):
    values = sorted(values)
    return values[len(values) // 2]


def thin():
    rng = np.random.default_rng(5)
    a = np.zeros((N, N, N), np.uint8)
    for _ in range(300):
        rad = int(rng.integers(8, 21))
        c = rng.integers(rad, N - rad, size=3)
        zz, yy, xx = np.mgrid[-rad:rad + 1, -rad:rad + 1, -rad:rad + 1]
        a[c[0] - rad:c[0] + rad + 1, c[1] - rad:c[1] + rad + 1, c[2] - rad:c[2] + rad + 1][zz * zz + yy * yy + xx * xx <= rad * rad] = 200
    return a


def thick():
    z, y, x = np.ogrid[:N, :N, :N]
    return np.where((z - 128) ** 2 + (y - 128) ** 2 + (x - 128) ** 2 <= 100 * 100, 200, 0).astype(np.uint8)


WORKLOADS = {'thin': thin, 'thick': thick}


def phases(profiles, names):
    return {name: median(p[name] for p in profiles) for name in names}


def run_thickness(workload):
    import vpt_amd
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, WORKLOADS[workload]())
    d = src.distance(100, 255, 'rest')
    reports, row = [], {}
    for _ in range(RUNS):
        t, report = d.thickness_timed()
        reports.append(report)
        row.update(tiles=report['tiles'], visited=report['visited'], largest=t.info['largest'], centres=N ** 3 - t.info['seeds'])
        t.destroy()
    t, uncut = d.thickness_timed(_flags=1)                        # once: without the value cull a thick structure takes seconds
    t.destroy()
    row['ms'] = phases([r['ms'] for r in reports[1:]], ('tiles', 'cover', 'info'))
    row['ms_total'] = median(sum(r['ms'].values()) for r in reports[1:])
    row['visited_per_tile'] = row['visited'] / max(row['tiles'], 1)
    row['visited_per_tile_without_value_cull'] = uncut['visited'] / max(row['tiles'], 1)
    row['ms_cover_without_value_cull'] = uncut['ms']['cover']
    d.destroy(); src.destroy(); ctx.destroy()
    return row


def run_distance(workload):
    import vpt_amd
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, WORKLOADS[workload]())
    profiles = []
    for _ in range(RUNS):
        d = src.distance(100, 255, 'rest')
        profiles.append(d.profile())
        d.destroy()
    row = {'ms': phases(profiles[1:], ('x', 'y', 'z')), 'ms_total': median(sum(p.values()) for p in profiles[1:])}
    src.destroy(); ctx.destroy()
    return row


STEPS = {'thickness': run_thickness, 'distance': run_distance}


def child(step, workload, limit, tree):
    """the JSON a child process of this script prints last, or None when it failed or ran out of time"""
    try:
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--workload", workload] +
                             (["--parent-tree", os.path.abspath(tree)] if tree else []), stdout=subprocess.PIPE, timeout=limit)
    except subprocess.TimeoutExpired:
        print("step %r of %r ran out of its %d s" % (step, workload, limit), file=sys.stderr)
        return None
    if res.returncode != 0:
        print("step %r of %r ended with %d" % (step, workload, res.returncode), file=sys.stderr)
        return None
    return json.loads(res.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit for the distance rows")
    ap.add_argument("--step", default=None, help="(internal) one of %s" % ", ".join(STEPS))
    ap.add_argument("--workload", default=None, help="(internal) one of %s" % ", ".join(WORKLOADS))
    a = ap.parse_args()
    if a.step is not None:
        if a.parent_tree:
            sys.path.insert(0, a.parent_tree)                     # in front of this tree: vpt_amd is the parent's
        print(json.dumps(STEPS[a.step](a.workload)))
        return 0
    out = {"volume": "256^3 R8, distances to the rest of the codes 100 .. 255; thin: 300 random balls of radii 8 .. 20 (seed 5); thick: one ball of radius 100",
           "timing": "the library's own phase times, the stream drained at the end of each phase; median of 5 after a warm-up (the run without the "
                     "value cull: one call); a fresh process per configuration; clocks not pinned.  'tiles' holds the host's sort of the tile list "
                     "and its upload; ms_total is the sum of the phases: the allocations in front of them are in neither",
           "distance_tree": "the parent commit's" if a.parent_tree else "this tree's",
           "not_measured": ["R16", "volumes beyond 256^3", "the Node.js host", "hardware counters", "seeds 'range' (the complement's thickness)"]}
    for workload in WORKLOADS:
        out[workload] = {}
        for step in STEPS:
            row = child(step, workload, a.step_timeout, a.parent_tree if step == 'distance' else "")
            if row is None:
                return 1
            out[workload][step] = row
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
