#!/usr/bin/env python3
"""Times of the 2x reduction and the binomial smoothing on the device (vpt_volume_reduce, vpt_volume_smooth), per size and format, beside
the yardsticks taken in the same run: the device's streaming-read rate (vpt_probe_stream_read), the finalize alone of each result
(vpt_volume_finalize of a volume of that size and format) and the gradient channel by central differences on the same volume
(vpt_volume_derive_gradient: the kernel whose form k_smooth follows).

    python tools/pyramid_rate.py [--out profiles/pyramid_rates.json] [--sizes 512 1024] [--kernel-trace TRACE.csv]

Min of 5 timed runs after a warm-up, the context synchronised around each.  Volume.reduce() / Volume.smooth(1) as a whole = allocation of
the result, the kernel and the finalize of the result.  The kernels' own times come from a separate
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/pyramid_rate.py` run of this script; --kernel-trace reads that run's
*_kernel_trace.csv and adds, per kernel and grid, the shortest dispatch and the rate at the algorithmic traffic: (1 + 1/8) B / 8 bytes per
source voxel for k_reduce, 2 B / 8 bytes per voxel and pass for k_smooth, 3 B / 8 for k_gradient (B in, 2 B out), each also as a fraction
of the streaming-read rate."""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpt_amd                                                     # noqa: E402
from vpt_amd import _native as N                                   # noqa: E402

FORMATS = (("R8", np.uint8), ("R16", np.uint16))


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
    """uniform noise over the low 12 bits (uint16) or every code (uint8): one random slab repeated along z (the rates do not depend on the data)"""
    rng = np.random.default_rng(n)
    slab = rng.integers(0, 4096 if dtype == np.uint16 else 256, size=(32, n, n)).astype(dtype)
    return np.ascontiguousarray(np.tile(slab, (n // 32, 1, 1)))


def finalize_us(ctx, vol, dtype):
    """the finalize alone of `vol` (one texel re-uploaded marks it dirty)"""
    L = N.lib()
    blk = np.zeros((1, 1, 1), dtype)
    times = []
    for _ in range(6):
        N.check(L.vpt_volume_upload_block(vol.getTexture(), 0, 0, 0, 1, 1, 1, blk.ctypes.data_as(C.c_void_p), blk.nbytes))
        ctx.synchronize()
        t0 = time.perf_counter()
        N.check(L.vpt_volume_finalize(vol.getTexture()))
        ctx.synchronize()
        times.append(time.perf_counter() - t0)
    return min(times[1:]) * 1e6


def kernel_times(path):
    """{(short kernel name, workgroups): shortest dispatch in us} from a rocprofv3 kernel trace"""
    best = {}
    with open(path, newline='') as f:
        for row in csv.DictReader(f):
            name = row.get("Kernel_Name", "")
            m = re.search(r"(k_reduce<[^>]*>|k_smooth<[^>]*>|k_gradient<[^>]*>)", name)
            if not m:
                continue
            grid = [int(row.get(k, 1) or 1) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z")]
            wg = [int(row.get(k, 1) or 1) for k in ("Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z")]
            groups = 1
            for g, w in zip(grid, wg):
                groups *= max(1, g // max(1, w))
            us = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3
            key = (m.group(1), groups)
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
    out = {"stream_read_GB_per_s": probe, "cases": {}}
    trace = kernel_times(a.kernel_trace) if a.kernel_trace else {}
    for n in a.sizes:
        for name, dtype in FORMATS:
            vol = source(dtype, n)
            b = vol.dtype.itemsize
            src = vpt_amd.Volume.from_array(ctx, vol, 'linear', norm16=dtype == np.uint16)
            del vol
            row = {}

            def reduce():
                return src.reduce().destroy
            row["reduce_us"] = timed(ctx, reduce) * 1e6

            def smooth():
                return src.smooth(1).destroy
            row["smooth1_us"] = timed(ctx, smooth) * 1e6

            def gradient():
                return src.derive_gradient('central').destroy
            row["gradient_central_us"] = timed(ctx, gradient) * 1e6
            r = src.reduce()
            row["finalize_reduced_us"] = finalize_us(ctx, r, dtype)
            r.destroy()
            s = src.smooth(1)
            row["finalize_smoothed_us"] = finalize_us(ctx, s, dtype)
            s.destroy()
            src.destroy()
            if trace:
                # the grids of this case: k_reduce one lane per 16 result bytes, k_smooth / k_gradient one workgroup per 128 x 8 x 32 voxels
                tiles = ((n + 127) // 128) * ((n + 7) // 8) * ((n + 31) // 32)
                chunks = n * b // 32 * (n // 2) * (n // 2)
                grids = {"k_reduce": (chunks + 255) // 256, "k_smooth": tiles, "k_gradient": tiles}
                traffic = {"k_reduce": (1 + 1 / 8) * b * n ** 3, "k_smooth": 2 * b * n ** 3, "k_gradient": 3 * b * n ** 3}
                t_tag = {np.uint8: ("unsigned char", "0,"), np.uint16: ("unsigned short", "1,")}[dtype]
                for (kernel, groups), us in sorted(trace.items()):
                    short = kernel.split("<")[0]
                    args = kernel.split("<", 1)[1]
                    mine = args.replace(" ", "").startswith(t_tag[1]) if short == "k_reduce" else args.startswith(t_tag[0])
                    if groups != grids[short] or not mine or (short == "k_gradient" and not re.match(r"[^,]*, *0,", args)):
                        continue
                    rate = traffic[short] / us / 1e3
                    row[short + "_us"] = us
                    row[short + "_GB_per_s"] = rate
                    row[short + "_fraction_of_stream_read"] = rate / probe
            out["cases"]["%d^3 %s" % (n, name)] = row
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.destroy()


if __name__ == "__main__":
    main()
