#!/usr/bin/env python3
"""Phase times of the isosurface mesh (vpt_volume_surface) on the device at 256^3 R8 (DESIGN.md "Surface"):

  thin    the project's 300 random overlapping balls (radii 8 .. 20), level 100: many small closed surfaces
  thick   one ball of radius 100, level 100: one large smooth surface
  noise   uniform random codes, level 128: nearly every cell is active, the output's bandwidth bounds it

For each: the counts of vpt_surface_info and the five phases of vpt_surface_profile (inside plane, classify, prefix sums, emit vertices,
emit quads); and beside them, as the scales to read the figures against, vpt_volume_components (26-connected, the codes 100 .. 255) on the
same input, and vpt_probe_stream_read of the volume's byte count (the inside-plane pass reads the volume once).

    python tools/surface_rate.py [--out profiles/surface_rates.json] [--step-timeout 300] [--parent-tree PATH]

--parent-tree: a built checkout of the parent commit; the components rows then import vpt_amd (and its library) from there, so that the
scale is the code as it stood before this unit.

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

import numpy as np                                                # noqa: E402

from thickness_rate import WORKLOADS as BALLS                     # noqa: E402  (the same two volumes)

RUNS = 6                                                          # a warm-up and five
PHASES = ('inside', 'classify', 'scan', 'vertices', 'quads')


def noise():
    return np.random.default_rng(5).integers(0, 256, (256, 256, 256), dtype=np.uint8)


WORKLOADS = {'thin': (BALLS['thin'], 100), 'thick': (BALLS['thick'], 100), 'noise': (noise, 128)}


def spread(values):
    values = sorted(values)
    return {'median': values[len(values) // 2], 'min': values[0], 'max': values[-1]}


def run_surface(workload):
    import vpt_amd
    make, level = WORKLOADS[workload]
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, make())
    profiles, row = [], {}
    for _ in range(RUNS):
        s = src.surface(level)
        profiles.append(s.profile)
        row.update(info=s.info)
        s.destroy()
    row['ms'] = {name: spread([p[name] for p in profiles[1:]]) for name in PHASES}
    row['ms_total'] = spread([sum(p.values()) for p in profiles[1:]])
    row['inside_gb_per_s'] = 256 ** 3 / (row['ms']['inside']['median'] * 1e6)
    out_bytes = 12 * row['info']['vertices'] + 16 * row['info']['quads']
    row['emit_gb_per_s'] = out_bytes / ((row['ms']['vertices']['median'] + row['ms']['quads']['median']) * 1e6)
    src.destroy(); ctx.destroy()
    return row


def run_components(workload):
    import vpt_amd
    ctx = vpt_amd.Context(0)
    src = vpt_amd.Volume.from_array(ctx, WORKLOADS[workload][0]())
    totals, listed = [], 0
    for _ in range(RUNS):
        c = src.components(100, 255, 26)
        totals.append(sum(c.profile()[0].values()))
        listed = c.info['listed']
        c.destroy()
    src.destroy(); ctx.destroy()
    return {'ms_total': spread(totals[1:]), 'listed': listed}


def run_probe(workload):
    import vpt_amd
    ctx = vpt_amd.Context(0)
    rates = [ctx.stream_read_rate(256 ** 3, 20) for _ in range(RUNS)]
    ctx.destroy()
    return {'gb_per_s': spread(rates[1:]), 'bytes': 256 ** 3}


STEPS = {'surface': run_surface, 'components': run_components, 'stream_read': run_probe}


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
    ap.add_argument("--parent-tree", default="", help="a built checkout of the parent commit for the components rows")
    ap.add_argument("--step", default=None, help="(internal) one of %s" % ", ".join(STEPS))
    ap.add_argument("--workload", default=None, help="(internal) one of %s" % ", ".join(WORKLOADS))
    a = ap.parse_args()
    if a.step is not None:
        if a.parent_tree:
            sys.path.insert(0, a.parent_tree)                     # in front of this tree: vpt_amd is the parent's
        print(json.dumps(STEPS[a.step](a.workload)))
        return 0
    out = {"volume": "256^3 R8; thin: 300 random balls of radii 8 .. 20 (seed 5), level 100; thick: one ball of radius 100, level 100; "
                     "noise: uniform random codes (seed 5), level 128",
           "timing": "the library's own phase times, the stream drained at the end of each phase; median, least and largest of 5 after a "
                     "warm-up; a fresh process per configuration; clocks not pinned.  ms_total is the sum of the phases: the allocations "
                     "(scratch in front of the first phase, the result in front of the emit) are in none.  components: all seven phases, connectivity 26, the codes 100 .. 255; "
                     "stream_read: vpt_probe_stream_read of 256^3 bytes, 20 iterations a call",
           "scale_tree": "the parent commit's" if a.parent_tree else "this tree's",
           "not_measured": ["R16 and two-channel volumes", "volumes beyond 256^3", "the Node.js host", "hardware counters"]}
    for workload in WORKLOADS:
        out[workload] = {}
        for step in ('surface', 'components'):
            row = child(step, workload, a.step_timeout, a.parent_tree if step == 'components' else "")
            if row is None:
                return 1
            out[workload][step] = row
    out['stream_read'] = child('stream_read', 'noise', a.step_timeout, "")
    if out['stream_read'] is None:
        return 1
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
