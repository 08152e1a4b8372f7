#!/usr/bin/env python3
"""Where a wave of the MISS-tile kernel (k_mcm_miss_settled / k_mcm_miss on the tiles the cube does not project onto) spends its life,
measured by an INSTRUMENTED build of the library: make -C vpt_amd/csrc OUT=../../build/ab/timing.so EXTRA=-DVPT_EVENT_TIMING (the
sibling of tools/r04_event_timing.py: the same per-wave slots, the same 100 MHz wave clock, each read behind the s_waitcnt of what the
phase produced).  Three phases per wave: the prologue up to the first event, the pass's events, the epilogue (state store) — with the
MISS kernel alone on the chip (one stream: HIT, then MISS) and beside the HIT-tile kernel (two streams, the default form).
Writes <out>_alone.json and <out>_beside_hit.json."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default="build/ab/timing.so")
ap.add_argument("--tag", default="", help="names the build in the output (for instance: parent order | prologue ahead of the barrier)")
ap.add_argument("--out", default="build/miss_wave_life")
ap.add_argument("--volume", type=int, default=512)
ap.add_argument("--frames", type=int, default=200)
ap.add_argument("--settled", default="1,0", help="VPT_OPTION_SETTLED_MISS values to run: 2 = k_mcm_miss_packed (the headline's), 1 = k_mcm_miss_settled, 0 = k_mcm_miss")
ap.add_argument("--order", default="wave", choices=["wave", "workgroup"],
                help="what the prologue's slots 1-5 of the build mean: 'wave' = the plain variants' order without a workgroup barrier "
                     "(vpt_kernels_mcm.h miss_wave_start); 'workgroup' = a build from before it (staged table, barrier)")
args = ap.parse_args()
SLOTS = {"wave": ["kernel_arguments_and_tile_list_entry_scalar_loads", "ndc_table_loads_flight_alpha_column_and_state_behind_them",
                  "pixel_constants_seed_alpha_column_writes", "state_texel_flight_left_after_the_arithmetic",
                  "photon_start_and_rest_up_to_the_first_event"],
         "workgroup": ["kernel_arguments_and_tile_list_entry_scalar_loads", "state_ndc_table_and_transfer_function_loads_flight",
                       "pixel_constants_seed_photon_start", "wait_at_the_workgroup_barrier", "rest_up_to_the_first_event"]}
os.environ["VPT_HIP_LIBRARY"] = os.path.abspath(args.lib)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import vpt_amd
from vpt_amd import _native as N
from vpt_amd.scene import default_camera, Transform, Node
from vpt_amd.synthetic import sphere_volume, GoldenRatioRng

W, H = 1920, 1080


def volume(n):
    cache = "/tmp/vpt_vol_%d.npy" % n                              # (shared with tools/ab_mcm.py)
    if os.path.exists(cache):
        return np.load(cache)
    from concurrent.futures import ThreadPoolExecutor
    v = np.empty((n, n, n), dtype=np.uint8)

    def slab(z0):
        v[z0:z0 + 16] = sphere_volume(n, noise=48.0, z_range=(z0, min(n, z0 + 16)))
    with ThreadPoolExecutor(max_workers=min(14, len(os.sched_getaffinity(0)))) as ex:
        list(ex.map(slab, range(0, n, 16)))
    np.save(cache, v)
    return v


def timing(r, name):
    out = (C.c_uint64 * 17)()
    f = getattr(N.lib(), name)
    f.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    f.restype = C.c_int
    N.check(f(r._h, out))
    return [int(x) for x in out]


ctx = vpt_amd.Context(0)
gvol = vpt_amd.Volume.from_array(ctx, volume(args.volume), 'linear')
results = {1: [], 2: []}
for fast in (1, 0):
    for settled in [int(x) for x in args.settled.split(",")]:
        for split in (1, 2):
            r = vpt_amd.MCMRenderer(ctx, gvol, default_camera(W / H), None, {'resolution': (W, H), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
            r.set_option(N.OPTION_FAST_MATH, fast)
            r.set_option(N.OPTION_SPLIT_STREAMS, split)
            r.set_option(N.OPTION_TILE_CLASSES, 2)                  # 2: the class kernels on one stream as well (HIT, then MISS: each alone on the chip)
            r.set_option(N.OPTION_SETTLED_MISS, settled)
            r.reset()
            hit, miss, _ = r.tile_classes()
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.3:
                for _ in range(50):
                    r.render()
                ctx.synchronize()
            timing(r, "vpt_probe_miss_timing"); timing(r, "vpt_probe_event_timing")     # clear
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.frames):
                r.render()
            ctx.synchronize()
            wall = (time.perf_counter() - t0) / args.frames * 1e6
            t = timing(r, "vpt_probe_miss_timing")
            th = timing(r, "vpt_probe_event_timing")
            waves = max(t[8], 1)
            parts = [10.0 * t[k] / waves for k in (1, 2, 3, 4, 5)]
            pro, ev, epi = sum(parts), 10.0 * t[0] / waves, 10.0 * t[6] / waves
            life = pro + ev + epi
            entry = {"build": args.tag or os.path.basename(args.lib), "volume": args.volume, "arithmetic": "fast-math" if fast else "bit-exact",
                     "miss_kernel": "k_mcm_miss_settled" if settled else "k_mcm_miss",
                     "form": "alone on the chip (one stream: HIT, then MISS)" if split == 1 else "beside the HIT-tile kernel (two streams)",
                     "hit_tiles": hit, "miss_tiles": miss, "miss_waves_per_frame": waves / args.frames, "settled_passes": r.settled_passes(),
                     "frame_us_wall_instrumented": wall,
                     "miss_wave_ns": {"prologue_up_to_the_first_event": pro, "events": ev, "epilogue_state_store": epi, "life": life},
                     "prologue_ns": dict(zip(SLOTS[args.order], parts)),
                     "share_of_life": {"prologue": pro / life, "events": ev / life, "epilogue": epi / life},
                     "hit_wave_life_ns_instrumented": 10.0 * sum(th[:8]) / max(th[8], 1),
                     "last_launch_timeline_us_after_the_first_miss_wave_started": {
                         "waves": t[9], "wave_start_p50_p90_max": [t[10] / 100.0, t[11] / 100.0, t[12] / 100.0],
                         "wave_end_p10_p50_p90_max": [t[13] / 100.0, t[14] / 100.0, t[15] / 100.0, t[16] / 100.0]}}
            results[split].append(entry)
            print(json.dumps(entry), flush=True)
            r.destroy()
gvol.destroy()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
for split, name in ((1, "alone"), (2, "beside_hit")):
    json.dump({"_what": __doc__.strip().split("\n\n")[0].replace("\n", " "),
               "_unit": "nanoseconds per MISS wave (10 ns clock ticks x 10), means over every MISS wave of %d frames" % args.frames,
               "_note": "the marks wait for vmcnt / lgkmcnt, so the instrumented kernel serialises what the shipped one overlaps at the three phase "
                        "borders; read the shares, not the frame time",
               "configs": results[split]}, open("%s_%s.json" % (args.out, name), "w"), indent=1)
ctx.destroy()
