#!/usr/bin/env python3
"""ms per frame of MCM and MCS lit by environment maps of growing size — the default 1x1, a 2048x1024 RGBA8 map, a 2048x1024 and an 8192x4096
HDR (RGBE8) map — on a 512^3 synthetic volume at 1920x1080, and the time vpt_renderer_set_environment_texels takes for the 8192x4096 map as
RGBE8 (128 MB over the bus) and as RGBA32F (512 MB).  The renderers of one kind live side by side; after a warm-up the maps alternate,
`--rounds` times, and the medians are printed as one JSON line.
Usage: python tools/envmap_rate.py [--size 512] [--frames 20] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sky(h, w, seed):
    """RGBE bytes of a smooth bright sky (exponents 126 .. 137: radiance up to ~4) with a little noise"""
    rng = np.random.default_rng(seed)
    y = np.linspace(0, 1, h, dtype=np.float32)[:, None]
    x = np.linspace(0, 1, w, dtype=np.float32)[None, :]
    out = np.empty((h, w, 4), np.uint8)
    out[..., 0] = (128 + 100 * y + 20 * x).astype(np.uint8)
    out[..., 1] = (160 + 60 * y).astype(np.uint8)
    out[..., 2] = (200 + 40 * x).astype(np.uint8)
    out[..., 3] = (126 + 11 * (1 - y)).astype(np.uint8)
    out[..., :3] ^= rng.integers(0, 4, size=(h, w, 3), dtype=np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--uploads", type=int, default=5)
    args = ap.parse_args()
    import vpt_amd
    from vpt_amd.hdr import HDRImage
    from vpt_amd.scene import default_camera, Transform, Node
    from vpt_amd.synthetic import colour_tf, sphere_volume, GoldenRatioRng
    W, H = args.width, args.height
    ctx = vpt_amd.Context(0)
    vol = vpt_amd.Volume.from_array(ctx, sphere_volume(args.size, noise=40.0))
    tf = colour_tf(256)
    big = sky(4096, 8192, 1)
    maps = {'1x1': None,
            '2048x1024 RGBA8': np.random.default_rng(2).integers(0, 256, size=(1024, 2048, 4), dtype=np.uint8),
            '2048x1024 RGBE8': HDRImage(sky(1024, 2048, 3), 2048, 1024),
            '8192x4096 RGBE8': HDRImage(big, 8192, 4096)}
    line = {"volume": args.size, "image": [W, H], "ms_per_frame": {}}
    for kind, cls in (('mcm', vpt_amd.MCMRenderer), ('mcs', vpt_amd.MCSRenderer)):
        rs = {}
        for name, env in maps.items():
            r = cls(ctx, vol, default_camera(W / H), env, {'resolution': (W, H), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
            r.setTransferFunction(tf)
            r.reset()
            for _ in range(args.warmup):
                r.render()
            rs[name] = r
        ctx.synchronize()
        times = {name: [] for name in rs}
        for _ in range(args.rounds):
            for name, r in rs.items():
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.frames):
                    r.render()
                ctx.synchronize()
                times[name].append((time.perf_counter() - t0) / args.frames * 1e3)
        line["ms_per_frame"][kind] = {k: round(statistics.median(v), 4) for k, v in times.items()}
        for r in rs.values():
            r.destroy()
    # upload + decode of the 8192 x 4096 map (the call returns once the table is on the device)
    r = vpt_amd.MCMRenderer(ctx, vol, default_camera(W / H), None, {'resolution': (64, 64), 'transform': Transform(Node())})
    f32 = np.empty(big.shape, np.float32)
    e = big[..., 3].astype(np.int32)
    f32[..., :3] = np.ldexp(big[..., :3].astype(np.float32), (e - 136)[..., None]); f32[..., 3] = 1.0
    line["upload_ms_8192x4096"] = {}
    for name, env in (('RGBE8', HDRImage(big, 8192, 4096)), ('RGBA32F', f32)):
        ts = []
        for _ in range(args.uploads):
            ctx.synchronize()
            t0 = time.perf_counter()
            r.setEnvironmentMap(env)
            ts.append((time.perf_counter() - t0) * 1e3)
        line["upload_ms_8192x4096"][name] = round(statistics.median(ts), 2)
    r.destroy()
    print(json.dumps(line), flush=True)
    vol.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
