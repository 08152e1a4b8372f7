#!/usr/bin/env python3
"""Times, launches and tile visits of the thinning on the device at 256^3 R8 (DESIGN.md "Skeleton"), the two workloads of
tools/thickness_rate.py:

  thin    the project's 300 random overlapping balls (radii 8 .. 20): many small structures
  thick   one ball of radius 100: one structure that takes about a hundred passes

For each, in mode 'ends' to the fixed point: the passes, the kernel launches, the tile visits of the sub-step launches with the tile cull
and (one run) without it, and the four phases of vpt_skeleton_profile (seed, border marking, sub-steps, census; the passes' times summed);
and beside them, as the scale to read the figures against, vpt_volume_distance and vpt_volume_components on the same input.

    python tools/skeleton_rate.py [--out profiles/skeleton_rates.json] [--step-timeout 300] [--parent-tree PATH]

--parent-tree: a built checkout of the parent commit; the distance and components rows then import vpt_amd (and its library) from there,
so that the scale is the code as it stood before this unit.

Each configuration runs in a child process of its own under its own time limit; the first that fails or runs out of time ends the run and
nothing further is started.  A figure is the median of 5 timed calls after a warm-up, with the least and the largest of the five beside
it; the times are the library's own (a phase up to the drained stream)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from thickness_rate import WORKLOADS                              # noqa: E402  (the same two volumes)

RUNS = 6                                                          # a warm-up and five
MODE = 'ends'


def spread(values):
    values = sorted(values)
    return {'median': values[len(values) // 2], 'min': values[0], 'max': values[-1]}


def run_skeleton(workload):
    import vpt_amd
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, WORKLOADS[workload]())
    profiles, row = [], {}
    for _ in range(RUNS):
        k = src.skeleton(100, 255, MODE)
        ms, launches, tiles = k.profile()
        profiles.append(ms)
        row.update(info=k.info, launches=launches, tile_visits=tiles)
        k.destroy()
    k = src.skeleton(100, 255, MODE, _flags=1)                    # once: every tile in every pass
    ms, _, tiles = k.profile()
    row['tile_visits_without_cull'] = tiles
    row['ms_steps_without_cull'] = ms['steps']
    k.destroy()
    row['ms'] = {name: spread([p[name] for p in profiles[1:]]) for name in ('seed', 'border', 'steps', 'census')}
    row['ms_total'] = spread([sum(p.values()) for p in profiles[1:]])
    row['us_per_launch'] = 1000.0 * row['ms_total']['median'] / row['launches']
    src.destroy(); ctx.destroy()
    return row


def run_distance(workload):
    import vpt_amd
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, WORKLOADS[workload]())
    totals = []
    for _ in range(RUNS):
        d = src.distance(100, 255, 'rest')
        totals.append(sum(d.profile().values()))
        d.destroy()
    src.destroy(); ctx.destroy()
    return {'ms_total': spread(totals[1:])}


def run_components(workload):
    import vpt_amd
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, WORKLOADS[workload]())
    totals, listed = [], 0
    for _ in range(RUNS):
        c = src.components(100, 255, 26)
        totals.append(sum(c.profile()[0].values()))
        listed = c.info['listed']
        c.destroy()
    src.destroy(); ctx.destroy()
    return {'ms_total': spread(totals[1:]), 'listed': listed}


STEPS = {'skeleton': run_skeleton, 'distance': run_distance, 'components': run_components}


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
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit for the distance and components rows")
    ap.add_argument("--step", default=None, help="(internal) one of %s" % ", ".join(STEPS))
    ap.add_argument("--workload", default=None, help="(internal) one of %s" % ", ".join(WORKLOADS))
    a = ap.parse_args()
    if a.step is not None:
        if a.parent_tree:
            sys.path.insert(0, a.parent_tree)                     # in front of this tree: vpt_amd is the parent's
        print(json.dumps(STEPS[a.step](a.workload)))
        return 0
    out = {"volume": "256^3 R8, the codes 100 .. 255, mode 'ends' to the fixed point; thin: 300 random balls of radii 8 .. 20 (seed 5); thick: one ball of radius 100",
           "timing": "the library's own phase times, the stream drained at the end of each phase (after the border launch and after the eight "
                     "sub-step launches of every pass); median, least and largest of 5 after a warm-up (the run without the tile cull: one call); "
                     "a fresh process per configuration; clocks not pinned.  ms_total is the sum of the phases: the allocations in front of "
                     "them are in neither.  distance: x + y + z passes; components: all seven phases, connectivity 26",
           "scale_tree": "the parent commit's" if a.parent_tree else "this tree's",
           "not_measured": ["R16", "volumes beyond 256^3", "modes 'kernel' and 'isthmus'", "the Node.js host", "hardware counters"]}
    for workload in WORKLOADS:
        out[workload] = {}
        for step in STEPS:
            row = child(step, workload, a.step_timeout, a.parent_tree if step != 'skeleton' else "")
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
