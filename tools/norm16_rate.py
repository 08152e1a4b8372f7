#!/usr/bin/env python3
"""ms per frame and volume samples per second of one synthetic field stored as R8 (c >> 8), R16 (c) and R32F (c / 65535): MIP, EAM, MCS,
MCM (bit-exact and fast math) and ISO at 1920x1080.  The three volumes and their renderers live side by side; after a warm-up the formats
alternate, `--rounds` times, and the median of each (renderer, format) is printed, one JSON line per volume size.
Usage: python tools/norm16_rate.py [--sizes 512 1024] [--frames 20] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RENDERERS = ('mip', 'eam', 'mcs', 'mcm', 'mcm_fast', 'iso')


def field16(n):
    """uint16 [n][n][n]: the noisy sphere of the benchmark in the high byte, a smooth ramp in the low byte (slab by slab)"""
    from vpt_amd.synthetic import sphere_volume
    out = np.empty((n, n, n), np.uint16)
    x = np.arange(n, dtype=np.uint16)
    for z0 in range(0, n, 64):
        z1 = min(n, z0 + 64)
        hi = sphere_volume(n, noise=40.0, z_range=(z0, z1)).astype(np.uint16) << 8
        lo = ((x[None, None, :] * 7 + np.arange(z0, z1, dtype=np.uint16)[:, None, None] * 3 + x[:n, None][None] * 5) & 255).astype(np.uint16)
        out[z0:z1] = hi | lo
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--renderers", nargs="+", default=list(RENDERERS))
    args = ap.parse_args()
    import vpt_amd
    from vpt_amd import _native as N
    from vpt_amd.scene import default_camera, Transform, Node
    from vpt_amd.synthetic import colour_tf, GoldenRatioRng
    W, H = args.width, args.height
    ctx = vpt_amd.Context(0)
    tf = colour_tf(256)
    classes = {'mip': vpt_amd.MIPRenderer, 'eam': vpt_amd.EAMRenderer, 'mcs': vpt_amd.MCSRenderer, 'mcm': vpt_amd.MCMRenderer,
               'mcm_fast': vpt_amd.MCMRenderer, 'iso': vpt_amd.ISORenderer}
    for n in args.sizes:
        c = field16(n)
        vols = {'R8': vpt_amd.Volume.from_array(ctx, (c >> 8).astype(np.uint8)),
                'R16': vpt_amd.Volume.from_array(ctx, c, norm16=True)}
        f = np.empty(c.shape, np.float32)
        for z0 in range(0, n, 64):
            f[z0:z0 + 64] = (c[z0:z0 + 64].astype(np.float64) / 65535.0).astype(np.float32)
        del c
        vols['R32F'] = vpt_amd.Volume.from_array(ctx, f)
        del f
        line = {"volume": n, "image": [W, H], "bricked_MiB": {k: v.bricked_bytes() / 2 ** 20 for k, v in vols.items()},
                "ms_per_frame": {}, "G_samples_per_s": {}}
        for kind in args.renderers:
            rs = {}
            for name, v in vols.items():
                r = classes[kind](ctx, v, default_camera(W / H), None, {'resolution': (W, H), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
                r.setTransferFunction(tf)
                if kind == 'mcm_fast':
                    r.set_option(N.OPTION_FAST_MATH, 1)
                r.reset()
                for _ in range(args.warmup):
                    r.render()
                rs[name] = r
            ctx.synchronize()
            times = {name: [] for name in rs}
            rates = {name: [] for name in rs}
            for _ in range(args.rounds):
                for name, r in rs.items():
                    s0 = r.sample_count()
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.frames):
                        r.render()
                    ctx.synchronize()
                    dt = time.perf_counter() - t0
                    times[name].append(dt / args.frames * 1e3)
                    rates[name].append((r.sample_count() - s0) / dt / 1e9)
            line["ms_per_frame"][kind] = {k: round(statistics.median(v), 4) for k, v in times.items()}
            line["G_samples_per_s"][kind] = {k: round(statistics.median(v), 2) for k, v in rates.items()}
            for r in rs.values():
                r.destroy()
        print(json.dumps(line), flush=True)
        for v in vols.values():
            v.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
