#!/usr/bin/env python3
"""Times of the rank filters on the device (vpt_volume_rank: median, erode, dilate, open, close; one pass), per size and format, beside the
yardsticks taken in the same run: the device's streaming-read rate (vpt_probe_stream_read) and one pass of the binomial smoothing on the
same volume (vpt_volume_smooth: the kernel whose form both rank kernels follow).

    python tools/rank_rate.py [--out profiles/rank_rates.json] [--sizes 512 1024] [--kernel-trace TRACE.csv]

Min of 5 timed runs after a warm-up, the context synchronised around each, uniform noise.  A whole call = allocation of the result (and of
the scratch volume for open / close, which are two launches), the kernels and the finalize of the result.  The kernels' own times come
from a separate `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/rank_rate.py` run of this script; --kernel-trace
reads that run's *_kernel_trace.csv and adds, per kernel, the shortest dispatch and the rate at the algorithmic traffic, 2 B / 8 bytes per
voxel and pass, also as a fraction of the streaming-read rate and beside k_smooth's."""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpt_amd                                                     # noqa: E402
from vpt_amd.rank import OPERATORS                                 # noqa: E402

FORMATS = (("R8", np.uint8), ("R16", np.uint16))
# packed 16-bit compare-exchanges (a v_pk_min_u16 and a v_pk_max_u16, two voxels each) per voxel of k_median: 150 of the selection and the
# median of the last three (2) per voxel pair, 9 of the y-sorts a plane per four voxels (vpt_volume_rank.hip)
MEDIAN_COMPARE_EXCHANGES_PER_VOXEL = (150 + 2) / 2 + 9 / 4


def timed(ctx, fn, runs=6):
    times = []
    for _ in range(runs):
        ctx.synchronize()
        t0 = time.perf_counter()
        done = fn()
        ctx.synchronize()
        times.append(time.perf_counter() - t0)
        if done is not None:
            done()
    return min(times[1:])


def source(dtype, n):
    """uniform noise over every code: one random slab repeated along z with a plane's offset (no plane equals its neighbour)"""
    rng = np.random.default_rng(n)
    top = int(np.iinfo(dtype).max) + 1
    slab = rng.integers(0, top, size=(33, n, n)).astype(dtype)
    return np.ascontiguousarray(np.concatenate([slab] * (n // 33 + 1))[:n])


def kernel_times(path):
    """{(short kernel name, template arguments, workgroups): shortest dispatch in us} from a rocprofv3 kernel trace"""
    best = {}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            m = re.search(r"(k_rank_extreme|k_median|k_smooth)<([^>]*)>", row.get("Kernel_Name", ""))
            if not m:
                continue
            grid = [int(row.get(k, 1) or 1) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z")]
            wg = [int(row.get(k, 1) or 1) for k in ("Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z")]
            groups = 1
            for g, w in zip(grid, wg):
                groups *= max(1, g // max(1, w))
            us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            key = (m.group(1), m.group(2).replace(" ", ""), groups)
            best[key] = min(best.get(key, us), us)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--kernel-trace", default="", help="*_kernel_trace.csv of a rocprofv3 run of this script: adds the kernels' own times")
    a = ap.parse_args()
    ctx = vpt_amd.Context(0)
    probe = ctx.stream_read_rate(1 << 30, 5)
    out = {"stream_read_GB_per_s": probe, "median_compare_exchanges_per_voxel": MEDIAN_COMPARE_EXCHANGES_PER_VOXEL, "cases": {}}
    trace = kernel_times(a.kernel_trace) if a.kernel_trace else {}
    for n in a.sizes:
        for name, dtype in FORMATS:
            vol = source(dtype, n)
            b = vol.dtype.itemsize
            src = vpt_amd.Volume.from_array(ctx, vol, 'linear', norm16=dtype == np.uint16)
            del vol
            row = {}
            for op in OPERATORS:
                row[op + "1_us"] = timed(ctx, lambda: src.rank(op, 1).destroy) * 1e6
            row["smooth1_us"] = timed(ctx, lambda: src.smooth(1).destroy) * 1e6
            src.destroy()
            if trace:
                tiles = ((n + 127) // 128) * ((n + 7) // 8) * ((n + 31) // 32)       # one workgroup per 128 x 8 x 32 voxels, all three kernels
                traffic = 2 * b * n ** 3
                t_tag = {np.uint8: "unsignedchar", np.uint16: "unsignedshort"}[dtype]
                for (kernel, args, groups), us in sorted(trace.items()):
                    if groups != tiles or not args.startswith(t_tag):
                        continue
                    label = kernel if kernel != "k_rank_extreme" else kernel + ("_max" if args.split(",")[1] in ("true", "1") else "_min")
                    rate = traffic / us / 1e3
                    row[label + "_us"] = us
                    row[label + "_GB_per_s"] = rate
                    row[label + "_fraction_of_stream_read"] = rate / probe
                for label in ("k_rank_extreme_min", "k_rank_extreme_max", "k_median"):
                    if label + "_us" in row and "k_smooth_us" in row:
                        row[label + "_times_k_smooth"] = row[label + "_us"] / row["k_smooth_us"]
            out["cases"]["%d^3 %s" % (n, name)] = row
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.destroy()


if __name__ == "__main__":
    main()
