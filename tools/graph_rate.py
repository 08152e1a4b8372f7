#!/usr/bin/env python3
"""Times of the skeleton graph on the device at 256^3 R8 (DESIGN.md "Skeleton graph"), on the 'ends' skeletons of the two workloads of
tools/skeleton_rate.py:

  thin    the project's 300 random overlapping balls (radii 8 .. 20): about 22 thousand kept voxels
  thick   one ball of radius 100: a few hundred kept voxels

For each: the six phases of vpt_graph_profile (seed, classify, branch labelling, node labelling, links, host ordering), the wall time of
Skeleton.graph() and of one Graph.prune(20) with the stream drained behind it; and beside them, as the scale to read the figures
against, what a user could compose before this unit: Skeleton.volume() followed by one vpt_volume_components call at 26-connectivity on it.

    python tools/graph_rate.py [--out profiles/graph_rates.json] [--step-timeout 300] [--parent-tree PATH]

--parent-tree: a built checkout of the parent commit; the composed row then imports vpt_amd (and its library) from there, so that the scale
is the code as it stood before this unit.

Each configuration runs in a child process of its own under its own time limit; the first that fails or runs out of time ends the run and
nothing further is started.  A figure is the median of 5 timed calls after a warm-up, with the least and the largest of the five beside
it; the phase times are the library's own (a phase up to the drained stream), the wall times are the host's around a blocking call."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from thickness_rate import WORKLOADS                              # noqa: E402  (the same two volumes)

RUNS = 6                                                          # a warm-up and five
MODE = 'ends'
PHASES = ('seed', 'classify', 'branches', 'nodes', 'links', 'host')


def spread(values):
    values = sorted(values)
    return {'median': values[len(values) // 2], 'min': values[0], 'max': values[-1]}


def run_graph(workload):
    import vpt_amd
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, WORKLOADS[workload]())
    k = src.skeleton(100, 255, MODE)
    profiles, walls, prunes, row = [], [], [], {}
    for _ in range(RUNS):
        ctx.synchronize()
        t0 = time.perf_counter()
        g = k.graph()
        walls.append(1000.0 * (time.perf_counter() - t0))
        ms, launches = g.profile()
        profiles.append(ms)
        t0 = time.perf_counter()
        out = g.prune(20)
        ctx.synchronize()
        prunes.append(1000.0 * (time.perf_counter() - t0))
        row.update(info=g.info, launches=launches, dropped=int(vpt_amd.graph.dropped(g.branch_records(), 20).sum()))
        out.destroy(); g.destroy()
    row['ms'] = {name: spread([p[name] for p in profiles[1:]]) for name in PHASES}
    row['ms_phases_total'] = spread([sum(p.values()) for p in profiles[1:]])
    row['ms_wall_graph'] = spread(walls[1:])
    row['ms_wall_prune'] = spread(prunes[1:])
    k.destroy(); src.destroy(); ctx.destroy()
    return row


def run_composed(workload):
    """what could be composed before this unit: the skeleton as a volume, then its 26-components"""
    import vpt_amd
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, WORKLOADS[workload]())
    k = src.skeleton(100, 255, MODE)
    walls, labels, listed = [], [], 0
    for _ in range(RUNS):
        ctx.synchronize()
        t0 = time.perf_counter()
        v = k.volume()
        c = v.components(100, 255, 26)
        walls.append(1000.0 * (time.perf_counter() - t0))
        labels.append(sum(c.profile()[0].values()))
        listed = c.info['listed']
        c.destroy(); v.destroy()
    k.destroy(); src.destroy(); ctx.destroy()
    return {'ms_wall': spread(walls[1:]), 'ms_components_phases': spread(labels[1:]), 'listed': listed}


STEPS = {'graph': run_graph, 'composed': run_composed}


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
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit for the composed row")
    ap.add_argument("--step", default=None, help="(internal) one of %s" % ", ".join(STEPS))
    ap.add_argument("--workload", default=None, help="(internal) one of %s" % ", ".join(WORKLOADS))
    a = ap.parse_args()
    if a.step is not None:
        if a.parent_tree:
            sys.path.insert(0, a.parent_tree)                     # in front of this tree: vpt_amd is the parent's
        print(json.dumps(STEPS[a.step](a.workload)))
        return 0
    out = {"volume": "256^3 R8, the 'ends' skeleton of the codes 100 .. 255; thin: 300 random balls of radii 8 .. 20 (seed 5); thick: one ball of radius 100",
           "timing": "phases: the library's own times, the stream drained at the end of each; wall: the host's clock around the blocking call "
                     "(Skeleton.graph(); Graph.prune(20) and a drain; Skeleton.volume() and Volume.components(100, 255, 26)), allocations "
                     "included; median, least and largest of 5 after a warm-up; a fresh process per configuration; clocks not pinned",
           "scale_tree": "the parent commit's" if a.parent_tree else "this tree's",
           "not_measured": ["R16", "volumes beyond 256^3", "sets that are not thin", "the Node.js host", "hardware counters"]}
    for workload in WORKLOADS:
        out[workload] = {}
        for step in STEPS:
            row = child(step, workload, a.step_timeout, a.parent_tree if step == 'composed' else "")
            if row is None:
                return 1
            out[workload][step] = row
        out[workload]['graph_over_composed_wall'] = out[workload]['graph']['ms_wall_graph']['median'] / out[workload]['composed']['ms_wall']['median']
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
