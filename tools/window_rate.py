#!/usr/bin/env python3
"""Times of the value-range window on the device (vpt_volume_window, vpt_volume_range, vpt_volume_code_histogram), per size and
format pair, beside the yardsticks taken in the same run: the device's streaming-read rate (vpt_probe_stream_read), the finalize alone
of the result (vpt_volume_finalize of an R8 / R16 volume of that size), what the operation replaces (vpt_amd.window_texels on the host
plus creating and uploading the result) and, with --render, MCM and EAM frame times at 1080p on the R16 volume and on its windowed R8 twin.

    python tools/window_rate.py [--out profiles/window_rates.json] [--sizes 512 1024] [--render] [--no-host]

Min of 5 timed runs after a warm-up, the context synchronised around each.  Volume.window() as a whole = allocation of the result, k_window
and the finalize of the result.  The kernels' own times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/window_rate.py
--no-host` run (rows k_window<...>, k_range<...>, k_code_histogram<...>); GB/s there are at the algorithmic bytes: (Bsrc + Bout) / 8 per
voxel for k_window, Bsrc / 8 for the other two."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpt_amd                                                     # noqa: E402
from vpt_amd import _native as N                                   # noqa: E402
from vpt_amd.synthetic import colour_tf, GoldenRatioRng            # noqa: E402

# (name, numpy dtype, result format, window) — a 12-bit series in a 16-bit container, Hounsfield units, a float field
PAIRS = (("R16->R8", np.uint16, 'r8', (205, 3890)), ("R16->R16", np.uint16, 'r16', (205, 3890)),
         ("R16_SNORM->R8", np.int16, 'r8', (-200, 400)), ("R32F->R16", np.float32, 'r16', (-1.0, 1.0)))


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
    rng = np.random.default_rng(n)
    if dtype == np.float32:
        return rng.standard_normal((n, n, n), dtype=np.float32)
    if dtype == np.int16:
        return rng.integers(-1000, 3001, size=(n, n, n), dtype=np.int16)
    return rng.integers(0, 4096, size=(n, n, n), dtype=np.uint16)


def upload(ctx, a):
    return vpt_amd.Volume.from_array(ctx, a, 'linear', norm16=a.dtype in (np.uint16, np.int16))


def frame_us(ctx, vol, cls, frames=20):
    from vpt_amd.scene import Transform, Node, default_camera
    r = cls(ctx, vol, default_camera(1920 / 1080), None, {'resolution': (1920, 1080), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
    r.setTransferFunction(colour_tf(256))
    r.reset()
    for _ in range(4):
        r.render()

    def run():
        for _ in range(frames):
            r.render()
    dt = timed(ctx, run)
    r.destroy()
    return dt / frames * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--render", action="store_true", help="also MCM and EAM frame times on the 512^3 R16 volume and its R8 window")
    ap.add_argument("--no-host", action="store_true", help="skip the host path (seconds of numpy per case)")
    a = ap.parse_args()
    ctx = vpt_amd.Context(0)
    L = N.lib()
    out = {"stream_read_GB_per_s": ctx.stream_read_rate(1 << 30, 5), "cases": {}}
    for n in a.sizes:
        for name, dtype, fmt, (lo, hi) in PAIRS:
            vol = source(dtype, n)
            src = upload(ctx, vol)
            bs, bo = vol.dtype.itemsize, 1 if fmt == 'r8' else 2
            row = {}

            def window():
                w = src.window(lo, hi, fmt)
                return w.destroy
            dt = timed(ctx, window)
            row["window_us"] = dt * 1e6
            row["window_GB_per_s"] = (bs + bo) * n ** 3 / dt / 1e9
            def rng():
                src.range()
            dt = timed(ctx, rng)
            row["range_us"] = dt * 1e6
            row["range_GB_per_s"] = bs * n ** 3 / dt / 1e9
            if dtype != np.float32:
                def hist():
                    src.code_histogram()
                dt = timed(ctx, hist)
                row["code_histogram_us"] = dt * 1e6
                row["code_histogram_GB_per_s"] = bs * n ** 3 / dt / 1e9
            # the yardstick: finalize alone of the result (one texel re-uploaded marks it dirty)
            w = src.window(lo, hi, fmt)
            blk = np.zeros((1, 1, 1), np.uint8 if fmt == 'r8' else np.uint16)
            times = []
            for _ in range(6):
                N.check(L.vpt_volume_upload_block(w.getTexture(), 0, 0, 0, 1, 1, 1, blk.ctypes.data_as(C.c_void_p), blk.nbytes))
                ctx.synchronize()
                t0 = time.perf_counter()
                N.check(L.vpt_volume_finalize(w.getTexture()))
                ctx.synchronize()
                times.append(time.perf_counter() - t0)
            row["finalize_result_us"] = min(times[1:]) * 1e6
            w.destroy()
            if not a.no_host:                                      # what the operation replaces: numpy on the host and a second upload
                t0 = time.perf_counter()
                texels = vpt_amd.window_texels(vol, lo, hi, fmt)
                t1 = time.perf_counter()
                twin = upload(ctx, texels)
                ctx.synchronize()
                t2 = time.perf_counter()
                twin.destroy()
                row["host_window_texels_us"] = (t1 - t0) * 1e6
                row["host_upload_us"] = (t2 - t1) * 1e6
            if a.render and n == 512 and name == "R16->R8":
                w = src.window(lo, hi, fmt)
                for kind, cls in (("mcm", vpt_amd.MCMRenderer), ("eam", vpt_amd.EAMRenderer)):
                    row["%s_1080p_us_R16" % kind] = frame_us(ctx, src, cls)
                    row["%s_1080p_us_windowed_R8" % kind] = frame_us(ctx, w, cls)
                row["bricked_bytes_R16"] = src.bricked_bytes()
                row["bricked_bytes_windowed_R8"] = w.bricked_bytes()
                w.destroy()
            src.destroy()
            del vol
            out["cases"]["%d^3 %s" % (n, name)] = row
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.destroy()


if __name__ == "__main__":
    main()
