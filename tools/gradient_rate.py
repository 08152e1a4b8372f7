#!/usr/bin/env python3
"""Time of the device-side gradient-magnitude derivation (vpt_volume_derive_gradient: allocation of the RG volume, k_gradient, and
the finalize of the result), per size and operator, beside the finalize alone of an RG volume of that size (the yardstick: code that was
there before, moving 2 + 4 bytes per voxel against the stencil's 1 + 2) and the streaming-read rate of the device.

    python tools/gradient_rate.py [--out profiles/gradient_rates.json] [--sizes 128 256 512 1024]

Min of 5 timed runs after a warm-up, the context synchronised around each.  GB/s are at the algorithmic traffic of the stencil,
3 * (B / 8) bytes per voxel.  The stencil kernel's own time comes from `rocprofv3 --kernel-trace --stats -- python tools/gradient_rate.py`
(rows k_gradient<...>); a 128^3 run is launch-bound and says nothing about the kernel."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512, 1024])
    a = ap.parse_args()
    ctx = vpt_amd.Context(0)
    L = N.lib()
    out = {"stream_read_GB_per_s": ctx.stream_read_rate(1 << 30, 5), "cases": {}}
    cases = [(n, 8) for n in a.sizes] + ([(512, 16)] if 512 in a.sizes else [])
    for n, bits in cases:
        dtype = np.uint8 if bits == 8 else np.uint16
        vol = np.random.default_rng(n).integers(0, 1 << bits, size=(n, n, n), dtype=dtype)
        src = vpt_amd.Volume.from_array(ctx, vol, 'linear', norm16=bits == 16)
        del vol
        row = {}
        for operator in ('central', 'sobel'):
            def derive():
                g = src.derive_gradient(operator, 1.0)
                return g.destroy
            dt = timed(ctx, derive)
            row[operator] = {"derive_us": dt * 1e6, "GB_per_s": 3.0 * (bits // 8) * n ** 3 / dt / 1e9}
        # the yardstick: finalize alone of an RG volume of this size (one texel re-uploaded marks it dirty)
        g = src.derive_gradient('central', 1.0)
        blk = np.zeros((1, 1, 1, 2), dtype)

        def finalize():
            N.check(L.vpt_volume_finalize(g.getTexture()))
        times = []
        for _ in range(6):
            N.check(L.vpt_volume_upload_block(g.getTexture(), 0, 0, 0, 1, 1, 1, blk.ctypes.data_as(C.c_void_p), blk.nbytes))
            ctx.synchronize()
            t0 = time.perf_counter()
            finalize()
            ctx.synchronize()
            times.append(time.perf_counter() - t0)
        row["finalize_rg_us"] = min(times[1:]) * 1e6
        g.destroy(); src.destroy()
        out["cases"]["%d^3 R%d" % (n, bits)] = row
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.destroy()


if __name__ == "__main__":
    main()
