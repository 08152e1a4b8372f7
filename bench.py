#!/usr/bin/env python3
"""bench.py — headline metric: volume samples/s (+ ms/frame) of the MCM renderer, synthetic 512^3 volume at
1920x1080, on N MI355X of one node (BASELINE.json).  One "step" = one AbstractRenderer.render() of the MCM
renderer = one integrate pass of `steps`=8 delta-tracking events per pixel + _renderFrame (fused in one launch),
inputs resident in HBM.  For N > 1 the image plane is sharded into interleaved row blocks (total work fixed =
strong scaling) and every frame is gathered over RCCL (all_gather, overlapped with the next frame's kernel).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Prints ONE JSON line on rank 0 with a `roofline` object.  A plain run does only what that line's headline needs: set up, warm up, time
the K steps, write --dump-outputs, print.  --full also runs everything measured or checked beside it (FULL_ONLY below: the oracle frame
check, the HBM stream probe, each kernel alone, the CPU baselines, the other configurations; N > 1: the forms beside the line and the
single-GPU reference); each of those options given explicitly wins over either default.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

B_ALG_MCM = 24.0          # algorithmic bytes per volume sample: 8 * sizeof(u8) + (64 B read + 64 B write) / steps(8)
B_OWN_MCM = 22.0          # the same with this library's 56-byte photon state: 8 + (56 + 56) / 8
HBM_PEAK_GBS = 8000.0     # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
# Stated tolerance of the fast-arithmetic MCM variant against the contract oracle in the N = 1 frame check: per pixel, the maximum over the RGB
# channels of |radiance - oracle radiance| on the band's texels (radiance = running mean of path radiances, each in [0, 1]), after every pass
# played (~4 700 in the default run).  Pixels whose rays miss the cube must agree exactly in path count and to 1e-6 in value; of the pixels that
# cross it >= 95 % must have the oracle's path count (a comparison that falls within rounding flips a path's fate: measured 98.4 %), and the
# mean / 99.9th percentile / maximum of |d| must stay below 8e-6 / 1.2e-3 / 2e-3 — at most 10 x what the driver's round-3 run measured
# (8.5e-7 / 1.2e-4 / 1.7e-4, BENCH_r03.json `frame_check_kind`; round 3's bounds were 50-100 x) — DESIGN.md section 3.
FAST_MATH_BOUNDS = {"max_abs_d_missing": 1e-6, "min_equal_counts_crossing": 0.97, "mean_abs_d_crossing": 8e-6,
                    "p999_abs_d_crossing": 1.2e-3, "max_abs_d_crossing": 2e-3}
# VPT_OPTION_SPLIT_STREAMS as the library sets it by itself (vpt_core.hip default_split): what a run without --split-streams uses
DEFAULT_SPLIT = {"mcm": 2, "mip": 3, "eam": 3, "iso": 2, "depth": 3, "mcs": 2, "lao": 2}
DUMP_CAP_BYTES = 60 << 20  # --dump-outputs: at most this many bytes of arrays in all (below 64 MB with the .npy headers)
# options whose work the headline does not need: off in a plain run, these values with --full (an explicit value wins either way)
FULL_ONLY = {"check": 1, "stream_probe": 1, "kernels_alone": 1, "other_configs": 1, "cpu_baseline": 1,
             "bucket_form": 1, "display_form": 1, "cadence_form": 16}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline does not need (every option of FULL_ONLY on; default: a plain run, all of them off)")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--volume", type=int, default=512)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--renderer", default="mcm", choices=["mcm", "mcs", "eam", "mip", "iso", "depth", "lao"])
    ap.add_argument("--extinction", type=float, default=None)
    ap.add_argument("--repeats", type=int, default=1,
                    help="the K-step timed block (barrier + synchronize on both sides) is run this many times; the MEDIAN block is reported "
                         "(default 1: exactly --steps steps are timed); an untimed block of --steps steps, run the same way, goes first")
    ap.add_argument("--warmup-seconds", type=float, default=0.3, help="warm up for at least this long (and at least --warmup steps)")
    ap.add_argument("--other-configs", type=int, default=None,
                    help="N = 1: after the timed region also measure BASELINE.json's other single-GPU configurations (C2 EAM 256^3, C3 MCS 512^3, "
                         "C4 MCM 1024^3, all 1920x1080) and report them in `other_configs` (default: 1 with --full, else 0)")
    ap.add_argument("--cpu-baseline", type=int, default=None, help="N = 1: time the C and JS CPU oracles on the same workload (default: 1 with --full, else 0)")
    ap.add_argument("--cpu-threads", type=int, default=0)
    ap.add_argument("--check", type=int, default=None,
                    help="N = 1: replay the passes with the CPU oracle on a band of rows; N > 1: verify the gathered frame against rank-local rows "
                         "and the same frames rendered unsharded (default: 1 with --full, else 0; `frame_check` null when off)")
    ap.add_argument("--profile-kernel", type=int, default=-1,
                    help="HIP events around every n-th launch of the dominant kernel in the timed region (1 = every launch, 0 = none; default -1 = every "
                         "max(8, steps / 2)-th: an event pair costs its stream a few microseconds, 0.3-1 %% of a 20-step block when every 8th launch carries one)")
    ap.add_argument("--stream-probe", type=int, default=None,
                    help="also measure the HBM streaming-read rate (second roofline denominator; default: 1 with --full, else 0)")
    ap.add_argument("--fused", type=int, default=1, help="0: run the three hooks as separate launches (profiling aid)")
    ap.add_argument("--frames-per-launch", type=int, default=0,
                    help="frames enqueued per host call (vpt_*_play); 0 = 1 (frame by frame)")
    ap.add_argument("--fused-passes", type=int, default=0,
                    help="MCM, single GPU, with --frames-per-launch F (<= 16 for 2): 1 = one launch runs F passes with the photon state in "
                         "registers and shows the last (VPT_PLAY_FUSED); 2 = the same, every pass's frame written to the frame ring (VPT_PLAY_FRAMES)")
    ap.add_argument("--graph", type=int, default=1, help="replay frame sequences as a captured hipGraph (with --frames-per-launch > 1)")
    ap.add_argument("--watchdog", type=int, default=1500, help="abort if the whole run takes longer than this many seconds")
    ap.add_argument("--gather-root", default="auto",
                    help="native gather: rank that receives every frame (grouped ncclSend/ncclRecv); -1 = every rank (all_gather); "
                         "auto = time both during the warm-up (rank 0 receives the frame either way) and keep the faster")
    ap.add_argument("--gather", default="auto", choices=["auto", "native", "torch"],
                    help="frame gather for N > 1: 'torch' = torch.distributed all_gather_into_tensor in buckets of --frames-per-gather frames; "
                         "'native' = RCCL pipeline below the C ABI (vpt_gather_*), measured AFTER a complete torch.distributed measurement and "
                         "under --native-deadline (the faster line is printed); 'auto' (default) = native only if a PREFLIGHT passes: every rank "
                         "starts tests/two_rank_worker.py in a fresh child process — a small scene through the native pipeline with this world "
                         "size (gather to rank 0, all_gather, gather to the last rank; the gathered frames bit-compared with unsharded ones) — "
                         "so that a fault of the never-before-run multi-rank path costs a child, not the measurement; else torch")
    ap.add_argument("--safe-first", type=int, default=1,
                    help="N > 1 with the native gather: measure over torch.distributed's all_gather first, then the native pipeline "
                         "under --native-deadline; print the faster (or the first, if the native phase does not finish)")
    ap.add_argument("--native-deadline", type=int, default=150, help="seconds the native gather phase may take (see --safe-first)")
    ap.add_argument("--fast-math", type=int, default=1,
                    help="MCM: 1 = the fast-arithmetic kernel variant (VPT_OPTION_FAST_MATH: hardware rcp / rsq / log / sin / cos; "
                         "checked against the contract by tolerance, not bit for bit)")
    ap.add_argument("--boundary-atlas", type=int, default=1,
                    help="MCM: 0 = out-of-cube samples from the bricks as well (VPT_OPTION_BOUNDARY_ATLAS off; results identical)")
    ap.add_argument("--tile-classes", type=int, default=1,
                    help="MCM: 0 = every tile through the general kernel (VPT_OPTION_TILE_CLASSES off; results identical); 2 = the class kernels also on "
                         "one stream, one after the other (with --split-streams 1: each kernel alone on the chip, for profiles)")
    ap.add_argument("--column-records", type=int, default=-1,
                    help="MCM: VPT_OPTION_COLUMN_RECORDS 0 / 1 (in-cube samples from the apron bricks / the column records); -1 = the library's choice by volume size")
    ap.add_argument("--split-streams", type=int, default=0,
                    help="K >= 1 = VPT_OPTION_SPLIT_STREAMS (a pass as K parts on K HIP streams; results identical); 0 (default) = set nothing: the "
                         "library's own default (MCM: 2 = the HIT | MISS kernels of the tile classes)")
    ap.add_argument("--kernels-alone", type=int, default=None,
                    help="N = 1, MCM with tile classes: after the timed region run the two class kernels one after the other on one stream "
                         "(VPT_OPTION_TILE_CLASSES 2) and report each kernel's duration alone on the chip in roofline.per_kernel "
                         "(default: 1 with --full, else 0)")
    ap.add_argument("--bucket-kernel", type=int, default=0,
                    help="torch.distributed pipeline, MCM with tile classes: 1 = the line's pipeline runs every bucket of --frames-per-gather frames by ONE launch "
                         "per tile class (VPT_OPTION_BUCKET_KERNEL: photon state in registers across the bucket, launch gap and staging once per bucket); "
                         "0 = one launch per frame and class, as at N = 1 (the default: like for like with the single-GPU line)")
    ap.add_argument("--display-form", type=int, default=None,
                    help="N > 1: 1 = measure the torch.distributed pipeline once more gathering the frames AS THE TONE MAPPER SHOWS THEM (RGBA8 through the default "
                         "Artistic tone mapper, vpt_renderer_play_into_display: bucket kernels with the table in their frame store, half the bytes per xGMI link) and "
                         "report it beside the line (config.display_gather_form); never the line's `value` (default: 1 with --full, else 0)")
    ap.add_argument("--bucket-form", type=int, default=None,
                    help="N > 1: 1 = after the line's measurement, measure the torch.distributed pipeline once more with VPT_OPTION_BUCKET_KERNEL and report "
                         "it beside the line (config.bucket_kernel_form); never the line's `value` unless --bucket-kernel 1 (default: 1 with --full, else 0)")
    ap.add_argument("--cadence-form", type=int, default=None,
                    help="N > 1, MCM: D > 0 = measure once more with the frame gathered at a DISPLAY CADENCE: D passes accumulate on every rank by one launch "
                         "per tile class (VPT_PLAY_FUSED) and only the D-th frame is gathered (RGBA16F all_gather) - what a progressive renderer that shows "
                         "every D-th pass needs from xGMI: 1 / D of the line's bytes per pass.  Reported beside the line (config.display_cadence_form) with the "
                         "single-GPU figure of the same form; never the line's `value`; 0 = skip (default: 16 with --full, else 0)")
    ap.add_argument("--frames-per-gather", type=int, default=16,
                    help="torch.distributed pipeline: frames per all_gather (every frame is delivered, at most F - 1 frames later; one async "
                         "collective costs the host ~25 us whatever its size and a bucket's launches ~10 us per frame, against the ~17 us a "
                         "1/8 shard's kernels take: measured on a one-rank group with 1920x136 frames 27.2 / 23.3 / 22.8 us per frame at F = 4 / 8 / 16)")
    ap.add_argument("--force-dist", type=int, default=0, help="initialise RCCL and run the frame all_gather even with one rank")
    ap.add_argument("--rehearsal", type=int, default=0,
                    help="1 = N ranks on ONE GPU (every rank on device 0) with the collectives over gloo instead of RCCL, which refuses two ranks on one "
                         "device: runs the whole N > 1 control flow of this file (shards of every rank, buckets, frame checks, the forms beside the line) "
                         "where only one GPU exists.  The line says `rehearsal`; its figures are NOT measurements of anything")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the line's path computed in its last step, as the caller receives it (the "
                         "RGBA16F frame; N > 1: the gathered frame), to DIR/frame.npy in float32 (over %d MB: a fixed seeded sample of "
                         "its pixels, DIR/frame.npy + DIR/frame_pixels.npy).  The timed steps then start from a restarted accumulation "
                         "(reset, per-frame draws from the first), so that the same arguments give the same outputs whatever the "
                         "time-based warm-up ran" % (DUMP_CAP_BYTES >> 20))
    args = ap.parse_args(argv)
    for name, value in FULL_ONLY.items():
        if getattr(args, name) is None:
            setattr(args, name, value if args.full else 0)
    return args


def dump_outputs(outputs, directory, seed=0):
    """writes each array of `outputs` as <directory>/<name>.npy in float32.  Above DUMP_CAP_BYTES in all, each array keeps its share of
    the cap as a fixed seeded sample of its pixels (rows of the array flattened to [pixels][channels], sorted pixel order), their flat
    indices in <name>_pixels.npy (float64: exact)"""
    os.makedirs(directory, exist_ok=True)
    import numpy as np
    arrays = {k: np.asarray(v, dtype=np.float32) for k, v in outputs.items()}
    total = sum(a.nbytes for a in arrays.values())
    written = []
    for name, a in sorted(arrays.items()):
        if total > DUMP_CAP_BYTES:
            flat = a.reshape(-1, a.shape[-1]) if a.ndim > 1 else a.reshape(-1, 1)
            share = DUMP_CAP_BYTES * a.nbytes // total
            n = min(flat.shape[0], share // (flat.shape[1] * 4 + 8))
            pick = np.sort(np.random.default_rng(seed).choice(flat.shape[0], n, replace=False))
            np.save(os.path.join(directory, name + "_pixels.npy"), pick.astype(np.float64))
            a = flat[pick]
            written.append(name + "_pixels")
        np.save(os.path.join(directory, name + ".npy"), a)
        written.append(name)
    return written


def cpu_baseline(vol, args, matrix, tf):
    """The CPU oracle (C restatement, "port") timed on this host on a bounded sample of the same workload:
    MCM reset + P full-frame integrate passes of the same scene, OpenMP over rows."""
    from oracle import oracle as O
    import numpy as np
    cores = len(os.sched_getaffinity(0))
    threads = args.cpu_threads or min(128, cores)          # every core of the host this process may run on (cap 128, stated below)
    sc = O.OracleScene(vol, 'linear', tf=tf)
    w, h = args.width, args.height
    o = O.OracleRenderer('mcm', sc, w, h)
    fr = O.make_frame(w, h, matrix, seed=0.5, extinction=1.0, anisotropy=0.0, max_bounces=8, mcm_steps=8, nthreads=threads)
    o.reset(fr)
    fr.seed = 0.25
    o.integrate(fr)                       # untimed: page in the volume
    t0 = time.perf_counter()
    n = 0
    passes = 0
    while passes < 400 and (passes < 4 or time.perf_counter() - t0 < 4.0):      # a bounded sample: ~4 s of wall time on all cores
        fr.seed = float(np.float32((passes + 1) * 0.61803398875 % 1.0))
        n += o.integrate(fr)
        passes += 1
    dt = time.perf_counter() - t0
    # the same oracle on ONE thread, on the middle half of the rows of one more pass (per-core figure)
    f1 = O.make_frame(w, h, matrix, seed=0.75, extinction=1.0, anisotropy=0.0, max_bounces=8, mcm_steps=8, nthreads=1,
                      y0=h // 4, y1=h // 4 + h // 2)
    t1 = time.perf_counter()
    n1 = o.integrate(f1)
    dt1 = time.perf_counter() - t1
    return {"value": n / dt, "unit": "volume samples/s", "cores": threads, "kind": "port",
            "sample": "%d MCM integrate passes (steps=8) of the full %dx%d frame on the same %d^3 volume, "
                      "oracle/vpt_oracle.c with OpenMP over rows on %d of the host's %d cores (cap 128), %.2f s wall" % (passes, w, h, args.volume, threads, cores, dt),
            "single_thread": {"value": n1 / dt1, "cores": 1,
                              "sample": "one pass over rows %d..%d on one thread, %.2f s" % (h // 4, h // 4 + h // 2, dt1)}}


def cpu_baseline_js(vol, args, matrix):
    """The scalar JavaScript ray-march BASELINE.json asks for (oracle/js/raymarch.js, single thread, node): MCM reset +
    2 integrate passes over a centred band of rows of the same 1920x1080 frame / volume; samples/s of the band."""
    import shutil, subprocess, tempfile
    import numpy as np
    node = shutil.which("node")
    if node is None:
        return {"value": None, "unit": "volume samples/s", "cores": 0, "kind": "port", "sample": "node not installed"}
    w, h = args.width, args.height
    band = 96
    y0 = max(0, h // 2 - band // 2); y1 = min(h, y0 + band)
    with tempfile.TemporaryDirectory() as tmp:
        vol.tofile(os.path.join(tmp, "vol.raw"))
        job = {"kind": "mcm", "nx": args.volume, "ny": args.volume, "nz": args.volume, "width": w, "height": h,
               "steps": 8, "bounces": 8, "extinction": 1.0, "anisotropy": 0.0, "reset_seed": 0.5,
               "seeds": [float(np.float32((k + 1) * 0.61803398875 % 1.0)) for k in range(2)], "y0": y0, "y1": y1,
               "mvp_inverse_bits": np.asarray(matrix, np.float32).view(np.uint32).tolist(), "volume": os.path.join(tmp, "vol.raw")}
        json.dump(job, open(os.path.join(tmp, "job.json"), "w"))
        res = subprocess.run([node, os.path.join(ROOT, "oracle", "js", "raymarch.js"), os.path.join(tmp, "job.json")],
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        if res.returncode != 0:
            return {"value": None, "unit": "volume samples/s", "cores": 0, "kind": "port", "sample": "node failed: " + res.stderr.decode()[-200:]}
        info = json.loads(res.stdout.decode().strip().splitlines()[-1])
    return {"value": info["samples"] / info["seconds"], "unit": "volume samples/s", "cores": 1, "kind": "port",
            "sample": "scalar JS (node %s) MCM, 2 integrate passes (steps=8) over rows %d..%d of the %dx%d frame, same %d^3 volume, %.2f s"
                      % (subprocess.check_output([node, "--version"]).decode().strip(), y0, y1, w, h, args.volume, info["seconds"])}


def other_configs(ctx, gvol512, vol512, args, W, H, torch):
    """BASELINE.json's other single-GPU configurations, measured after the headline's timed region (so that the driver's record
    carries them): per config the median of 3 synchronised blocks of 100 render() calls.  frac = algorithmic bytes per sample
     x samples/s / 8 TB/s, as for the headline."""
    import numpy as np
    import vpt_amd
    from vpt_amd import _native as N
    from vpt_amd.scene import default_camera, Transform, Node
    from vpt_amd.synthetic import sphere_volume, GoldenRatioRng
    from concurrent.futures import ThreadPoolExecutor

    def run(kind, gvol, frames=100, camera_z=None, tf=None, **props):
        """split / classes None = the library's default (not set)"""
        cam = default_camera(W / H)
        if camera_z is not None:
            cam.transform.localTranslation = [0.0, 0.0, float(camera_z)]
        r = vpt_amd.RendererFactory(kind)(ctx, gvol, cam, None, {'resolution': (W, H), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
        if tf is not None:
            r.setTransferFunction(tf)
        for k, v in props.items():
            if v is None:
                continue
            if k == "fast_math":
                r.set_option(N.OPTION_FAST_MATH, int(v))
            elif k == "split":
                r.set_option(N.OPTION_SPLIT_STREAMS, int(v))
            elif k == "classes":
                r.set_option(N.OPTION_TILE_CLASSES, int(v))
            elif k == "records":
                r.set_option(N.OPTION_COLUMN_RECORDS, int(v))
            else:
                setattr(r, k, v)
        r.reset()
        state_["tiles"] = r.tile_classes()[:2] if kind in ("mcm", "mcs", "eam", "mip") else None
        # warm up by TIME, like the headline: creating the renderer (and a volume before it) leaves the GPU idle long enough to drop its clocks, and
        # the first ~0.2 s after that run 7 % slow (EAM on three streams 56.2 us from cold, 52.4 in steady state; back to 56.2 after 3 s of idling)
        t_w = time.perf_counter()
        while time.perf_counter() - t_w < 0.4:
            for _ in range(20):
                r.render()
            ctx.synchronize()
        blocks = []
        for _ in range(3):
            r.clear_sample_count()
            t0 = time.perf_counter()
            for _ in range(frames):
                r.render()
            ctx.synchronize()
            blocks.append((time.perf_counter() - t0, r.sample_count()))
        dt, ns = sorted(blocks)[1]
        if kind != "mcm":
            state_["tiles"] = r.tile_classes()[:2]                    # (the marchers build their lists with the second fused pass)
        r.destroy()
        return dt / frames, ns / frames

    state_ = {"tiles": None}
    out = {}
    try:
        v256 = sphere_volume(256, noise=48.0)
        g256 = vpt_amd.Volume.from_array(ctx, v256, 'linear')
        b = 8.0 + 12.0 / 64.0
        # (after the first frame since the reset a fused render() launches the tiles some ray of which can meet the cube only, DESIGN.md
        # section 5; the library's best form is three tile-list ranges on three streams)
        for name, sp, tc in (("C2_eam_256_1080p", None, None), ("C2_eam_256_1080p_one_stream", 1, 1), ("C2_eam_256_1080p_whole_image_launches_one_stream", 1, 0)):
            t, ns = run('eam', g256, split=sp, classes=tc)
            out[name] = {"ms_per_frame": t * 1e3, "samples_per_s": ns / t, "bytes_per_sample": b, "frac": b * ns / t / (HBM_PEAK_GBS * 1e9),
                         "tile_classes": tc is None or bool(tc), "streams": sp or DEFAULT_SPLIT["eam"], "options_set": [] if sp is None else ["split_streams", "tile_classes"]}
        g256.destroy()
        for name, sp in (("C3_mcs_512_1080p", None), ("C3_mcs_512_1080p_one_stream", 1)):
            t, ns = run('mcs', gvol512, split=sp)
            # algorithmic bytes per sample: 8 + 48 B of frame / accumulator traffic per pixel and pass — priced on the pixels a
            # pass actually LAUNCHES (after the first frame: the HIT tiles only; round 3 charged all W x H pixels for traffic not performed)
            tiles = state_["tiles"]
            launched = (tiles[0] * 256) if (tiles and tiles[1] > 0) else W * H
            b = 8.0 + 48.0 * launched / max(ns, 1e-9)
            out[name] = {"ms_per_frame": t * 1e3, "ms_per_256_spp": t * 256e3, "samples_per_s": ns / t, "samples_per_pixel_per_frame": ns / (W * H),
                         "pixels_launched_per_frame": launched, "hit_tiles": tiles[0] if tiles else None, "miss_tiles": tiles[1] if tiles else None,
                         "bytes_per_sample": b, "frac": b * ns / t / (HBM_PEAK_GBS * 1e9), "streams": sp or DEFAULT_SPLIT["mcs"]}
        # C3 asks for the image after 256 samples per pixel, not for its 256 intermediate frames: vpt_renderer_play(16, VPT_PLAY_FUSED) runs 16
        # passes per launch with the running mean in registers and writes the render buffer after the 16th — bit-identical to 16 render()
        # calls (tests/test_gpu_parity.py frame sequences); the frame-by-frame rows above are what the reference's own loop does
        r = vpt_amd.RendererFactory('mcs')(ctx, gvol512, default_camera(W / H), None, {'resolution': (W, H), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
        r.reset()
        t_w = time.perf_counter()
        while time.perf_counter() - t_w < 0.3:
            r.play(16, fused=True)
            ctx.synchronize()
        blocks = []
        for _ in range(3):
            r.clear_sample_count()
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(16):
                r.play(16, fused=True)
            ctx.synchronize()
            blocks.append((time.perf_counter() - t0, r.sample_count()))
        dt, ns = sorted(blocks)[1]
        r.destroy()
        out["C3_mcs_512_1080p_256_spp_in_16_launches"] = {"ms_per_256_spp": dt * 1e3, "ms_per_pass": dt / 256 * 1e3, "samples_per_s": ns / dt, "passes_per_launch": 16,
                                                          "note": "the converged image C3 names, without its intermediate frames: 16 passes per launch, one render-buffer write per launch"}
        n = 1024
        v = np.empty((n, n, n), dtype=np.uint8)

        def slab(z0):
            v[z0:z0 + 16] = sphere_volume(n, noise=48.0, z_range=(z0, z0 + 16))
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=min(14, len(os.sched_getaffinity(0)))) as ex:
            list(ex.map(slab, range(0, n, 16)))
        t_gen = time.perf_counter() - t0
        g1024 = vpt_amd.Volume.from_array(ctx, v, 'linear')
        del v
        # (MCM forms: tile classes on = HIT | MISS kernels on two streams, the library's best form; "_general_kernel" = every tile through
        # k_mcm_integrate as in round 2, on one or three streams)
        for name, fm, sp, tc, rec in (("C4_mcm_1024_1080p", 0, None, None, None), ("C4_mcm_1024_1080p_fast_math", 1, None, None, None),
                                      ("C4_mcm_1024_1080p_fast_math_bricks", 1, None, None, 0),
                                      ("C4_mcm_1024_1080p_general_kernel_one_stream", 0, 1, 0, None), ("C4_mcm_1024_1080p_fast_math_general_kernel_three_streams", 1, 3, 0, None)):
            t, ns = run('mcm', g1024, fast_math=fm, split=sp, classes=tc, records=rec)
            out[name] = {"ms_per_frame": t * 1e3, "samples_per_s": ns / t, "bytes_per_sample": B_ALG_MCM, "tile_classes": tc is None or bool(tc), "streams": sp or DEFAULT_SPLIT["mcm"],
                         "in_cube_samples_from": "apron bricks" if rec == 0 else "column records (the library's choice beyond 512 MiB of bricks)",
                         "roofline": {"frac": B_ALG_MCM * ns / t / (HBM_PEAK_GBS * 1e9), "achieved": B_ALG_MCM * ns / t / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s"}}
        out["C4_mcm_1024_1080p"]["volume_generate_s"] = t_gen
        g1024.destroy()
        # the headline workload in its other forms (the line above sets --fast-math 1 and nothing else: the library's defaults)
        for name, fm, sp, tc in (("H_mcm_512_1080p_bit_exact", 0, None, None), ("H_mcm_512_1080p_fast_math", 1, None, None),
                                 ("H_mcm_512_1080p_bit_exact_one_stream", 0, 1, 1), ("H_mcm_512_1080p_fast_math_one_stream", 1, 1, 1),
                                 ("H_mcm_512_1080p_bit_exact_general_kernel_one_stream", 0, 1, 0), ("H_mcm_512_1080p_bit_exact_general_kernel_three_streams", 0, 3, 0),
                                 ("H_mcm_512_1080p_fast_math_general_kernel_one_stream", 1, 1, 0), ("H_mcm_512_1080p_fast_math_general_kernel_three_streams", 1, 3, 0)):
            t, ns = run('mcm', gvol512, frames=200, fast_math=fm, split=sp, classes=tc)
            out[name] = {"ms_per_frame": t * 1e3, "samples_per_s": ns / t, "tile_classes": tc is None or bool(tc), "streams": sp or DEFAULT_SPLIT["mcm"],
                         "options_set": ["fast_math"] * fm + ([] if sp is None else ["split_streams", "tile_classes"]),
                         "roofline": {"frac": B_ALG_MCM * ns / t / (HBM_PEAK_GBS * 1e9)}}
        # What the library does when the headline frame is NOT 79 % sky and the medium not thin (the default scene: ~93 % of all events leave the
        # cube): (1) the camera moved to z = 0.9 — the volume's front face fills the frame, every tile is a HIT tile, no MISS-tile kernel runs;
        # (2) extinction 50 with the 256 x 1 grey-ramp transfer function (alpha = v): a dense medium, short free paths, most in-cube events scatter
        from vpt_amd.synthetic import ramp_tf
        for name, fm, kw in (("H_mcm_512_1080p_fast_math_every_tile_hit_camera_z_0.9", 1, {"camera_z": 0.9}),
                             ("H_mcm_512_1080p_bit_exact_every_tile_hit_camera_z_0.9", 0, {"camera_z": 0.9}),
                             ("H_mcm_512_1080p_fast_math_extinction_50_grey_ramp", 1, {"extinction": 50.0, "tf": ramp_tf(256)}),
                             ("H_mcm_512_1080p_bit_exact_extinction_50_grey_ramp", 0, {"extinction": 50.0, "tf": ramp_tf(256)})):
            t, ns = run('mcm', gvol512, frames=200, fast_math=fm, **kw)
            tiles = state_["tiles"]
            out[name] = {"ms_per_frame": t * 1e3, "samples_per_s": ns / t, "hit_tiles": tiles[0], "miss_tiles": tiles[1], "streams": DEFAULT_SPLIT["mcm"],
                         "options_set": ["fast_math"] * fm, "roofline": {"frac": B_ALG_MCM * ns / t / (HBM_PEAK_GBS * 1e9)}}
        # NOT the judged form: 16 passes per launch with the photon state in registers (VPT_PLAY_FUSED), the render buffer written
        # after the 16th only — a display mode ("show every 16th pass"); it says what the state round trip costs the judged form
        for name, fm in (("H_mcm_512_1080p_bit_exact_display_every_16th_pass", 0), ("H_mcm_512_1080p_fast_math_display_every_16th_pass", 1)):
            r = vpt_amd.RendererFactory('mcm')(ctx, gvol512, default_camera(W / H), None,
                                               {'resolution': (W, H), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
            r.set_option(N.OPTION_FAST_MATH, fm)
            r.reset()
            t_w = time.perf_counter()
            while time.perf_counter() - t_w < 0.4:
                r.play(16, fused=True)
                ctx.synchronize()
            blocks = []
            for _ in range(3):
                r.clear_sample_count()
                t0 = time.perf_counter()
                for _ in range(12):
                    r.play(16, fused=True)
                ctx.synchronize()
                blocks.append((time.perf_counter() - t0, r.sample_count()))
            dt, ns = sorted(blocks)[1]
            r.destroy()
            out[name] = {"ms_per_pass": dt / (12 * 16) * 1e3, "samples_per_s": ns / dt, "passes_per_launch": 16,
                         "note": "not the judged step: one launch = 16 passes, one render-buffer write"}
        # VPT_PLAY_FRAMES: 16 passes per launch with the state in registers, EVERY pass's frame written to the frame ring (what 16
        # render() calls would have shown); a sequence mode for callers that display or record frames later than they ask for them
        for name, fm in (("H_mcm_512_1080p_bit_exact_16_frames_per_launch_every_frame_written", 0),
                         ("H_mcm_512_1080p_fast_math_16_frames_per_launch_every_frame_written", 1)):
            r = vpt_amd.RendererFactory('mcm')(ctx, gvol512, default_camera(W / H), None,
                                               {'resolution': (W, H), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
            r.set_option(N.OPTION_FAST_MATH, fm)                  # (tile classes on two streams are the default: one launch per class, k_mcm_bucket_hit | k_mcm_bucket_miss)
            r.reset()
            t_w = time.perf_counter()
            while time.perf_counter() - t_w < 0.4:
                r.play(16, frames=True)
                ctx.synchronize()
            blocks = []
            for _ in range(3):
                r.clear_sample_count()
                t0 = time.perf_counter()
                for _ in range(12):
                    r.play(16, frames=True)
                ctx.synchronize()
                blocks.append((time.perf_counter() - t0, r.sample_count()))
            dt, ns = sorted(blocks)[1]
            r.destroy()
            out[name] = {"ms_per_frame": dt / (12 * 16) * 1e3, "samples_per_s": ns / dt, "frames_per_launch": 16,
                         "roofline": {"frac": B_ALG_MCM * ns / dt / (HBM_PEAK_GBS * 1e9)},
                         "note": "not the judged step (one render() per launch): one launch per tile class = 16 frames, each written to its ring slot, "
                                 "photon state read once and written once per launch"}
    except Exception as e:                              # reporting only: the headline line must still be printed
        out["error"] = repr(e)
    return out


def native_preflight(dist, torch, device, rank, world, local_rank, timeout=180):
    """Every rank runs tests/two_rank_worker.py in a fresh child process (its own process group on a port agreed here): the native RCCL
    gather pipeline on a small scene with THIS world size, bit-compared with unsharded frames.  Returns "ok" on every rank only if every
    child exited 0 in time; a child that hangs is killed (by its PID), one that crashes takes nothing with it."""
    import socket
    import subprocess
    port = [None]
    if rank == 0:
        with socket.socket() as s_:
            s_.bind(("127.0.0.1", 0)); port[0] = s_.getsockname()[1]
    dist.broadcast_object_list(port, src=0)
    env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(local_rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port[0]),
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    verdict = "ok"
    try:
        p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "two_rank_worker.py")], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        try:
            out, _ = p.communicate(timeout=timeout)
            if p.returncode != 0:
                verdict = "child of rank %d exited %d: %s" % (rank, p.returncode, out.decode(errors="replace")[-300:].replace("\n", " | "))
        except subprocess.TimeoutExpired:
            p.kill()
            p.communicate()
            verdict = "child of rank %d did not finish in %d s" % (rank, timeout)
    except OSError as e:
        verdict = "child of rank %d could not start: %r" % (rank, e)
    flag = torch.tensor([1 if verdict == "ok" else 0], dtype=torch.int32, device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    if int(flag[0]) == 0 and verdict == "ok":
        verdict = "another rank's child failed"
    return verdict


def main():
    args = parse()
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)              # a directory that cannot be made fails before the run, not after it
    if args.profile_kernel < 0:
        args.profile_kernel = max(8, args.steps // 2) | 1        # odd: the sampled launches do not sit at the same place of every timed block
        if args.steps % args.profile_kernel == 0:
            args.profile_kernel += 2
    # stdout carries exactly ONE line, the JSON: RCCL prints its version banner to stdout when a communicator comes up,
    # so everything before the result goes to stderr's descriptor
    sys.stdout.flush()
    real_stdout = os.dup(1)
    os.dup2(2, 1)
    # a collective that never completes must not hang the caller for ever: give up loudly
    import threading

    def _give_up():
        sys.stderr.write("bench.py: no result after %d s (a hung collective or kernel?) - aborting\n" % args.watchdog)
        sys.stderr.flush()
        os._exit(3)
    watchdog = threading.Timer(args.watchdog, _give_up)
    watchdog.daemon = True
    watchdog.start()
    state = {"fallback": None, "make_line": None, "stream_gbs": None}

    def _native_gave_up():
        # the library's own RCCL pipeline did not finish its measurement in time: report the torch.distributed one
        sys.stderr.write("bench.py: the native gather pipeline did not finish within %d s - reporting the torch.distributed measurement\n" % args.native_deadline)
        sys.stderr.flush()
        have_line = state["fallback"] is not None and state["make_line"] is not None
        if int(os.environ.get("RANK", "0")) == 0 and have_line:
            line = state["make_line"](state["fallback"])
            line["native_timeout"] = True
            line["config"]["note"] = "native RCCL gather pipeline timed out; torch.distributed all_gather measurement reported"
            os.write(real_stdout, (json.dumps(line) + "\n").encode())
        sys.stderr.write("bench.py: rank %s was in: %s\n" % (os.environ.get("RANK", "0"), state.get("phase", "?")))
        sys.stderr.flush()
        os._exit(0 if have_line else 4)               # the first (complete, frame-checked) measurement stands; only its absence is a failure
    lib_path = os.path.join(ROOT, "vpt_amd", "libvpt_hip.so")
    if not os.path.exists(lib_path):                       # git-ignored artefact: a bare checkout builds it (one rank, the others wait)
        if int(os.environ.get("LOCAL_RANK", "0")) == 0:
            import subprocess                              # in a child: build() loads the library, and here torch must load HIP first
            subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT, stdout=sys.stderr)
        else:
            for _ in range(600):
                if os.path.exists(lib_path):
                    break
                time.sleep(1.0)
    import numpy as np
    import torch                       # first: its libamdhip64 is the one libvpt_hip.so binds to
    import torch.distributed as dist
    import vpt_amd
    from vpt_amd import _native as N
    from vpt_amd.scene import default_camera, Transform, Node
    from vpt_amd.synthetic import sphere_volume, GoldenRatioRng
    from vpt_amd.tiles import FrameGather, RcclFrameGather

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run --nproc-per-node %d for --gpus %d" % (args.gpus, args.gpus))
    if args.rehearsal:
        local_rank = 0                                     # every rank on the box's one GPU
        args.gather = "torch"                              # the native pipeline is RCCL's; two ranks on one device are refused by it
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        if args.rehearsal:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)

    W, H = args.width, args.height
    vol = sphere_volume(args.volume, noise=48.0)
    stream = torch.cuda.Stream(device=device)
    with torch.cuda.stream(stream):
        ctx = vpt_amd.Context(local_rank, stream=stream.cuda_stream)
        gvol = vpt_amd.Volume.from_array(ctx, vol, 'linear')
        gather = FrameGather(dist, torch, W, H, device, always_collective=bool(args.force_dist), frames_per_gather=max(1, args.frames_per_gather))
        camera = default_camera(W / H)
        transform = Transform(Node())
        opts = {'resolution': (W, H), 'transform': transform, 'rng': GoldenRatioRng(), 'fused': bool(args.fused)}
        if world > 1:
            opts['shard'] = gather.shard()
        r = vpt_amd.RendererFactory(args.renderer)(ctx, gvol, camera, None, opts)
        if args.extinction is not None:
            r.extinction = args.extinction
        if args.renderer != "mcm":
            args.fast_math = 0                              # an MCM option
        if args.fast_math:
            r.set_option(N.OPTION_FAST_MATH, 1)
        # The default line sets ONE option, the arithmetic (--fast-math): tile classes, the HIT | MISS kernels on two streams and everything else
        # are the library's own defaults since round 4.  N > 1: the native pipeline keeps the two streams apart across frames (its communication
        # stream waits for both); the torch.distributed pipeline hands the library a bucket of --frames-per-gather frames per call
        # (vpt_renderer_play_into), whose passes run on both streams and are joined once, by the call itself, in front of the collective.
        # Without tile classes (--tile-classes 0, other renderers) more ranges only pay from ~500 rows of 1920 pixels on (round 2): those
        # runs stay on one stream below that size.
        classes_on = bool(args.tile_classes) and args.renderer == "mcm"
        if use_dist and not classes_on and int(r.local_rows()) * W < 500 * 1920 and args.split_streams == 0:
            args.split_streams = 1
        if args.split_streams >= 1:
            r.set_option(N.OPTION_SPLIT_STREAMS, args.split_streams)
        eff_split = args.split_streams if args.split_streams >= 1 else DEFAULT_SPLIT.get(args.renderer, 1)     # what the passes run on
        if not args.boundary_atlas and args.renderer == "mcm":
            r.set_option(N.OPTION_BOUNDARY_ATLAS, 0)
        if args.tile_classes != 1 and args.renderer == "mcm":
            r.set_option(N.OPTION_TILE_CLASSES, args.tile_classes)
        if args.column_records >= 0 and args.renderer == "mcm":
            r.set_option(N.OPTION_COLUMN_RECORDS, args.column_records)
        bucket_capable = bool(use_dist and classes_on and eff_split >= 2 and gather.F > 1 and args.fused)
        if args.bucket_kernel and bucket_capable:
            r.set_option(N.OPTION_BUCKET_KERNEL, 1)
        # which gather the steps below drive: the RGBA16F one, or (display form) an RGBA8 one fed by vpt_renderer_play_into_display
        pipe = {"gather": gather, "tm": None}
        assert r.local_rows() == gather.rows
        nbytes = gather.send[0].numel() * 2
        r.reset()
        native = None
        preflight = None
        if use_dist and args.gather == "auto":
            preflight = native_preflight(dist, torch, device, rank, world, local_rank) if (world > 1 or args.force_dist > 1) else "skipped: one rank"
            args.gather = "native" if preflight == "ok" else "torch"
            if rank == 0:
                print("native gather preflight: %s -> --gather %s" % (preflight, args.gather), file=sys.stderr)
        state["preflight"] = preflight
        if use_dist and args.gather == "native":
            # bootstrap the library's own RCCL communicator through torch.distributed; every rank must agree that it
            # came up, otherwise all of them fall back to the torch.distributed gather
            err = ""
            try:
                ids = [RcclFrameGather.unique_id() if rank == 0 else None]
                dist.broadcast_object_list(ids, src=0)
                native = RcclFrameGather(r, ids[0], rank, world, root=0 if args.gather_root == "auto" else int(args.gather_root))
            except Exception as e:                       # noqa: BLE001 - reported below
                err = repr(e)
            flag = torch.tensor([0 if native is not None else 1], dtype=torch.int32, device=device)
            dist.all_reduce(flag)
            if int(flag[0]) != 0:
                if native is not None:
                    native.destroy()
                native = None
                args.gather = "torch"
                if rank == 0:
                    print("native RCCL gather unavailable (%s); using torch.distributed all_gather" % err, file=sys.stderr)

        bucket_on = [bool(args.bucket_kernel and bucket_capable)]
        fpl = args.frames_per_launch or 1             # measured: sequences do not beat frame-by-frame enqueue
        if fpl > 1 and native is None and use_dist:
            fpl = 1                                   # the torch.distributed gather is driven frame by frame
        use_native = [native is not None]            # which gather pipeline the steps below drive

        def make_line(res):
            """the JSON line of one measurement (rank 0)"""
            per_launch_samples = res["samples_local"] / max(args.steps, 1)
            avg_ms = res["kernel_ms"] / res["launches"] if res["launches"] else res["dt"] / args.steps * 1e3
            event_ms = avg_ms
            buckets = bool(use_dist and not res["native"] and gather.F > 1 and args.fused)      # torch pipeline: vpt_renderer_play_into, split inside
            split = eff_split >= 2 and (not use_dist or res["native"] or buckets)
            if split:
                # a step is K launches (K tile-row ranges on K streams) that overlap each other and the next step's: a
                # per-launch duration no longer says what the chip does.  The chip-level rate is bytes of a step / time of a step.
                avg_ms = res["dt"] / args.steps * 1e3
            bps = B_ALG_MCM if args.renderer == "mcm" else 8.0
            achieved = bps * per_launch_samples / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
            traffic, valu_busy, traffic_source, bound_override, bound_note = None, None, None, None, None
            tj_all, key = None, None
            tpath = os.path.join(ROOT, "profiles", "traffic.json")
            classes = res.get("tile_classes")
            classified = bool(classes and classes[1] > 0)
            if os.path.exists(tpath):
                try:
                    tj = json.load(open(tpath)); tj_all = tj
                    key = "%s_%d_%dx%d_n%d%s%s" % (args.renderer, args.volume, W, H, world, "_fast" if args.fast_math else "", "_classes" if classified else "")
                    traffic = tj.get(key)
                    valu_busy = tj.get(key + "_valu_busy_frac")
                    bound_override, bound_note = tj.get(key + "_bound"), tj.get(key + "_bound_source")
                    if traffic is not None:
                        traffic_source = tj.get(key + "_source", "profiles/traffic.json: committed rocprofv3 --pmc passes of this configuration (not measured in this run)")
                except Exception:
                    traffic = None
            stream_gbs = state["stream_gbs"]
            f = fpl if (res["native"] or not use_dist) else 1
            if not use_dist:
                par = "single GPU"
            elif res["native"]:
                par = "image rows sharded over %d GPU(s), per-frame RCCL %s (native pipeline below the C ABI)" % (
                    world, ("gather to rank %d" % res["root"]) if res["root"] >= 0 else "all_gather")
            else:
                par = "image rows sharded over %d GPU(s), RCCL all_gather of every %d frames (torch.distributed pipeline)" % (world, gather.F)
            variant = "fast-math" if args.fast_math else "bit-exact"
            own_bps = bps
            kernels = None
            launches_per_step = eff_split if split else 1
            if args.renderer != "mcm":
                kernel_name = "k_%s<fused>" % args.renderer
            elif classified:
                ntiles = classes[0] + classes[1]
                own_bps = 8.0 + (112.0 * classes[0] + 64.0 * classes[1]) / ntiles / 8.0
                kernel_name = ("k_mcm_integrate<fused render, %s> on the %d HIT tiles | k_mcm_miss<fused render, %s> on the %d MISS tiles "
                               "(tile classes, DESIGN.md section 5)" % (variant, classes[0], variant, classes[1]))
                launches_per_step = 2 if not split else max(2, eff_split)
                side_ms = res["side_kernel_ms"] / res["side_launches"] if res.get("side_launches") else None
                kernels = [{"name": "k_mcm_integrate<fused render, %s>" % variant, "tiles": classes[0], "stream": "context",
                            "avg_ms_hip_events": event_ms, "samples_per_launch": per_launch_samples * classes[0] / ntiles},
                           {"name": "k_mcm_miss<fused render, %s>" % variant, "tiles": classes[1], "stream": "side 0" if split else "context",
                            "avg_ms_hip_events": side_ms, "samples_per_launch": per_launch_samples * classes[1] / ntiles}]
            else:
                own_bps = B_OWN_MCM
                kernel_name = "k_mcm_integrate<fused render, %s>" % variant
            if split:
                duration_source = ("timed block / steps: a step is %d launches on %d HIP streams that overlap each other and the next step's, so the chip-level "
                                   "duration of a step is the block's wall time / steps; HIP events around the context stream's launch alone read %.4f ms%s"
                                   % (launches_per_step, eff_split, event_ms,
                                      (", around the side stream's %.4f ms" % (res["side_kernel_ms"] / res["side_launches"])) if res.get("side_launches") else ""))
            else:
                duration_source = "HIP events around every %d-th launch on the kernel's stream" % max(args.profile_kernel, 1)
            line = {
                "metric": "volume samples/s, MCM %d^3 @ %dx%d" % (args.volume, W, H) if args.renderer == "mcm"
                          else "volume samples/s, %s %d^3 @ %dx%d" % (args.renderer.upper(), args.volume, W, H),
                "value": res["samples"] / res["dt_max"], "unit": "volume samples/s",
                "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": res["dt_max"] / args.steps * 1e3, "higher_is_better": True,
                "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                "config": {"workload": "%s renderer, synthetic %d^3 u8 volume (radial sphere + lattice noise), %dx%d, "
                                       "default camera, default 2x1 transfer function, extinction %g, anisotropy 0, bounces 8, "
                                       "steps 8 per pass, 1 pass per step" % (args.renderer.upper(), args.volume, W, H, float(r.extinction) if hasattr(r, 'extinction') else 0.0),
                           "parallelism": par,
                           "gather_calibration": res["gather_choice"], "native_preflight": state.get("preflight"),
                           "frames_per_gather": (gather.F if (use_dist and not res["native"]) else None),
                           "frames_per_launch": f, "hipgraph": bool(args.graph) and f > 1 and not res["native"] and not args.fused_passes,
                           "fused_passes": bool(args.fused_passes) and f > 1, "every_frame_written": (args.fused_passes == 2 and f > 1) or not (bool(args.fused_passes) and f > 1),
                           "samples_per_step": res["samples"] / args.steps,
                           "arithmetic": ("fast-math variant (VPT_OPTION_FAST_MATH: hardware rcp/rsq/sqrt/log/sin/cos; tolerance-checked against the "
                                          "contract oracle, tests/test_gpu_fast_math.py)" if args.fast_math else
                                          "bit-exact contract (every buffer identical to oracle/vpt_oracle.c)"),
                           "boundary_atlas": bool(args.boundary_atlas),
                           "tile_classes": (dict(zip(("hit_tiles", "miss_tiles"), r.tile_classes()[:2])) if (args.renderer == "mcm" and args.tile_classes) else None),
                           "split_streams": eff_split if split else 1, "split_streams_set_by": "--split-streams" if args.split_streams >= 1 else "library default",
                           "options_set": [o for o in (("VPT_OPTION_FAST_MATH=1" if args.fast_math else None),
                                                       ("VPT_OPTION_SPLIT_STREAMS=%d" % args.split_streams if args.split_streams >= 1 else None),
                                                       ("VPT_OPTION_TILE_CLASSES=%d" % args.tile_classes if (args.renderer == "mcm" and args.tile_classes != 1) else None),
                                                       ("VPT_OPTION_COLUMN_RECORDS=%d" % args.column_records if (args.renderer == "mcm" and args.column_records >= 0) else None),
                                                       ("VPT_OPTION_BOUNDARY_ATLAS=0" if (args.renderer == "mcm" and not args.boundary_atlas) else None)) if o],
                           "repeats": args.repeats, "block_ms_min": min(res["blocks_ms"]), "block_ms_max": max(res["blocks_ms"]),
                           "block_ms_median": res["dt"] * 1e3, "timed_block": "median of `repeats` blocks of `steps` steps"},
                # `frac` prices the kernel against the HBM roofline by ALGORITHMIC bytes, as the metric is defined; what actually
                # limits it is read off the PMC passes (profiles/): VALU issue (VALUBusy) for the MCM pass, not HBM
                "roofline": {"bound": bound_override or ("valu" if (valu_busy or 0) >= 0.7 else "hbm"), "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source, "valu_busy_frac": valu_busy,
                             "bound_source": bound_note or ("VALUBusy of the committed PMC passes (profiles/traffic.json): >= 0.7 reads as VALU-issue bound, the HBM "
                                                            "roofline is what `frac` prices the step against either way"),
                             "peak_measured_stream_read": stream_gbs,
                             "frac_of_measured": (achieved / stream_gbs) if stream_gbs else None,
                             "kernel": kernel_name, "kernels": kernels,
                             "kernel_avg_ms": avg_ms, "launches": res["launches"],
                             "launches_per_step": launches_per_step,
                             "duration_source": duration_source,
                             "bytes_per_sample": bps,
                             # the kernels' own photon-state layout: 56 B per pixel each way in HIT tiles, 32 B in MISS tiles (not the
                             # reference's 64): priced by the bytes they move themselves
                             "bytes_per_sample_own_layout": own_bps,
                             "frac_own_layout": achieved / HBM_PEAK_GBS * (own_bps / bps)},
                "frame_check": res["ok"],
            }
            if args.rehearsal:
                line["rehearsal"] = ("%d ranks on ONE GPU, collectives over gloo (--rehearsal 1): the N > 1 control flow only; none of this line's figures "
                                     "is a measurement" % world)
            alone = state.get("alone")
            if alone and kernels:
                # each class kernel ALONE on the chip (one stream, VPT_OPTION_TILE_CLASSES 2, measured after the timed region): its own fraction of
                # the algorithmic roofline, and the HBM traffic of the committed PMC passes over its algorithmic bytes
                tk = (tj_all.get(key + "_per_kernel") or {}) if tj_all else {}
                per = []
                for kk, which in zip(kernels, ("hit", "miss")):
                    us = alone.get(which + "_us")
                    spl = kk["samples_per_launch"]
                    tb = tk.get(which)
                    per.append({"name": kk["name"], "tiles": kk["tiles"], "samples_per_launch": spl, "alone_us": us,
                                "frac_alg": (bps * spl / (us * 1e-6) / 1e9 / HBM_PEAK_GBS) if us else None,
                                "traffic_ratio": (tb / (bps * spl)) if tb else None})
                line["roofline"]["per_kernel"] = per
                line["roofline"]["per_kernel_source"] = alone["how"] + "; traffic_ratio = HBM bytes per launch of the committed PMC passes (profiles/traffic.json) / (24 B x samples)"
            if res.get("frame_check_kind"):
                line["frame_check_kind"] = res["frame_check_kind"]
            if "other_pipeline_ms_per_step" in res:
                line["config"]["other_pipeline_ms_per_step"] = res["other_pipeline_ms_per_step"]
            line["config"]["bucket_kernel"] = bool(res.get("bucket_kernel"))
            if state.get("bucket_form"):
                line["config"]["bucket_kernel_form"] = state["bucket_form"]
            if state.get("single_gpu"):
                sg = state["single_gpu"]
                line["config"]["single_gpu_reference"] = sg
                ratios = {"line_vs_single_gpu_frame_by_frame": sg["frame_by_frame_ms"] / line["ms_per_step"]}
                if state.get("bucket_form"):
                    ratios["bucket_kernel_form_vs_single_gpu_bucket_kernels"] = sg["bucket_kernels_16_frames_per_launch_ms"] / state["bucket_form"]["ms_per_step"]
                    ratios["bucket_kernel_form_vs_single_gpu_frame_by_frame"] = sg["frame_by_frame_ms"] / state["bucket_form"]["ms_per_step"]
                line["config"]["speedup_like_for_like"] = ratios
            if state.get("display_form"):
                line["config"]["display_gather_form"] = state["display_form"]
            if state.get("cadence_form"):
                line["config"]["display_cadence_form"] = state["cadence_form"]
                sg = state.get("single_gpu")
                if sg and sg.get("display_cadence_ms_per_pass"):
                    line["config"].setdefault("speedup_like_for_like", {})["display_cadence_form_vs_single_gpu_same_form"] = (
                        sg["display_cadence_ms_per_pass"] / state["cadence_form"]["ms_per_pass"])
            return line
        state["make_line"] = make_line

        def step_many(n):
            """n frames by one native call: per-frame uniforms in a device table, optionally one hipGraph replay"""
            if use_native[0]:
                native.play(n, fused=bool(args.fused_passes))   # no graph mode: graphs holding RCCL collectives are slower here
            else:
                r.play(n, use_graph=bool(args.graph) and n == fpl, fused=bool(args.fused_passes) and args.fused_passes != 2,
                       frames=args.fused_passes == 2)    # one cached graph: only full-size chunks replay it

        def step(k):
            if use_native[0]:
                native.render()                      # kernel + async RCCL all_gather, one enqueue each, below the C ABI
                return
            if not use_dist:
                r.render()                           # one GPU: the renderer's own render buffer, nothing to exchange
                return
            g = pipe["gather"]
            if pipe["tm"] is not None:
                r.play_into_display(pipe["tm"], 1, g.acquire().data_ptr(), nbytes // 2)
                g.commit()
                return
            r.play_into(1, g.acquire().data_ptr(), nbytes)         # the next slot of the current bucket (the call joins its own streams)
            g.commit()                               # a full bucket of --frames-per-gather frames: one all_gather

        def drain():
            if use_native[0]:
                native.synchronize()
            else:
                pipe["gather"].flush(); pipe["gather"].wait_all()

        frames_done = [0]

        def run_steps(nsteps):
            frames_done[0] += nsteps
            f = fpl if (use_native[0] or not use_dist) else 1
            if use_dist and not use_native[0] and gather.F > 1 and args.fused:
                # torch.distributed pipeline: whole buckets by ONE native call each (vpt_renderer_play_into: frame i into slot i of the
                # bucket), one caller-side join, one collective; a remainder goes frame by frame
                done = 0
                g = pipe["gather"]
                while done < nsteps:
                    bucket = g.acquire_bucket() if nsteps - done >= g.F else None
                    if bucket is None:
                        step(done); done += 1
                        continue
                    if pipe["tm"] is not None:
                        r.play_into_display(pipe["tm"], g.F, bucket.data_ptr(), nbytes // 2)
                    else:
                        r.play_into(g.F, bucket.data_ptr(), nbytes)
                    g.commit_bucket()                          # (the call has joined the bucket's streams in front of this collective)
                    done += g.F
                return
            if f <= 1:
                for k in range(nsteps):
                    step(k)
                return
            done = 0
            while done < nsteps:
                n = min(f, nsteps - done)
                if n == 1:
                    step(done)
                else:
                    step_many(n)
                done += n

        def single_gpu_frame_check():
            """N = 1: every pass played so far, replayed by the CPU oracle on a 4-row band with the same seed sequence; the final
            radiance + sample-count texels of the band must be bit-identical (contract arithmetic) or statistically equal
            (fast-math variant: same path counts on >= 97 % of the pixels, mean |difference| below the Monte-Carlo noise)"""
            from oracle import oracle as O
            y0, y1 = H // 2 - 2, H // 2 + 2
            sc = O.OracleScene(vol, 'linear')
            o = O.OracleRenderer('mcm', sc, W, H)
            rng = GoldenRatioRng()
            m = r._matrix()
            nthreads = min(64, len(os.sched_getaffinity(0)))
            fr = O.make_frame(W, H, m, seed=np.float32(rng()), extinction=float(r.extinction), anisotropy=0.0, max_bounces=8, mcm_steps=8,
                              y0=y0, y1=y1, nthreads=nthreads)
            o.reset(fr)
            for _ in range(frames_done[0]):
                fr.seed = float(np.float32(rng()))
                o.integrate(fr)
            want = o.state[3].reshape(H, W, 4)[y0:y1]
            got = r.read(N.BUFFER_MCM_RADIANCE)[y0:y1]
            if not args.fast_math:
                return bool((got.view(np.uint32) == want.view(np.uint32)).all()), "oracle band rows %d..%d after %d passes, bit-identical" % (y0, y1, frames_done[0])
            # The fast-arithmetic variant has no bit-exact twin.  What is asserted (bounds = FAST_MATH_BOUNDS; per pixel and
            # per channel, on the band's radiance texels after every pass played):
            #   * pixels whose paths never meet the cube (every event completes a path: count = 8 per pass, exactly): the same count
            #     and |d| within rounding of the running mean;
            #   * pixels that cross the cube (the ~21 % that the figure is about): equal path counts on >= min_equal_counts of them,
            #     mean / 99.9th percentile / maximum of the per-pixel max-channel |d| below the stated bounds
            full = 8.0 * frames_done[0]
            crossing = want[..., 3] < full
            d = np.abs(got[..., :3].astype(np.float64) - want[..., :3].astype(np.float64)).max(axis=-1)
            dc, dm = d[crossing], d[~crossing]
            stats = {"pixels_crossing_the_cube": int(crossing.sum()), "pixels_missing_it": int((~crossing).sum()),
                     "equal_counts_crossing": float((got[..., 3] == want[..., 3])[crossing].mean()) if crossing.any() else 1.0,
                     "equal_counts_missing": float((got[..., 3] == want[..., 3])[~crossing].mean()) if (~crossing).any() else 1.0,
                     "mean_abs_d_crossing": float(dc.mean()) if dc.size else 0.0, "p999_abs_d_crossing": float(np.quantile(dc, 0.999)) if dc.size else 0.0,
                     "max_abs_d_crossing": float(dc.max()) if dc.size else 0.0, "max_abs_d_missing": float(dm.max()) if dm.size else 0.0}
            B = FAST_MATH_BOUNDS
            ok = (stats["equal_counts_missing"] == 1.0 and stats["max_abs_d_missing"] <= B["max_abs_d_missing"] and
                  stats["equal_counts_crossing"] >= B["min_equal_counts_crossing"] and stats["mean_abs_d_crossing"] <= B["mean_abs_d_crossing"] and
                  stats["p999_abs_d_crossing"] <= B["p999_abs_d_crossing"] and stats["max_abs_d_crossing"] <= B["max_abs_d_crossing"])
            return bool(ok), {"what": "oracle band rows %d..%d after %d passes; fast-math variant against the contract oracle, per pixel, max over the "
                                      "RGB channels of |radiance difference|" % (y0, y1, frames_done[0]), "measured": stats, "bounds": B}

        def last_outputs():
            """what a caller of the timed path receives from its last step: the frame (N = 1: the renderer's texture; N > 1: the
            gathered frame, rank 0), as float32"""
            if use_native[0]:
                frame = native.frame() if native.receives() else None
            elif use_dist:
                frame = pipe["gather"].last_frame().cpu().numpy()
            else:
                frame = r.getTexture()
            return {} if frame is None else {"frame": frame.astype(np.float32)}

        def measure():
            """W warm-up steps (and >= --warmup-seconds), one untimed block of K steps, then --repeats blocks of EXACTLY K timed steps between barriers; the median
            block, max over ranks; the frame checked (N = 1: oracle band; N > 1: the gathered frame)"""
            res = {"native": use_native[0], "gather_choice": None, "bucket_kernel": bucket_on[0] and not use_native[0]}
            launches0 = r.bucket_launches() if args.renderer == "mcm" else 0
            r.set_profiling(args.profile_kernel)          # before the warm-up so that a captured graph carries its timing events
            if use_native[0] and args.gather_root == "auto":
                # which exchange is faster on this node is a property of RCCL's p2p and collective paths: measure both
                trial = {}
                for root in (0, -1):
                    native.set_root(root)
                    run_steps(8); drain(); dist.barrier(); torch.cuda.synchronize()
                    t_ = time.perf_counter()
                    run_steps(40); drain(); torch.cuda.synchronize()
                    tt_ = torch.tensor([time.perf_counter() - t_], dtype=torch.float64, device=device)
                    dist.all_reduce(tt_, op=dist.ReduceOp.MAX)
                    trial[root] = float(tt_[0]) / 40
                best = min(trial, key=trial.get)
                native.set_root(best)
                res["gather_choice"] = {"chosen_root": best, "ms_per_frame_root0": trial[0] * 1e3, "ms_per_frame_all_gather": trial[-1] * 1e3}
            run_steps(args.warmup)                        # the first frame sequence runs eagerly (lazy allocations) ...
            if fpl > 1 and (use_native[0] or not use_dist):
                run_steps(2 * fpl)                        # ... the next ones capture and replay the graph, outside the timed region
            drain()
            torch.cuda.synchronize()
            # warm up by TIME as well (clocks, caches, the Infinity Cache's share of the photon state): a cold box gave the
            # driver 0.154 ms where a warm one measures 0.144 ms.  Every rank runs the same number of extra steps.
            t_w = time.perf_counter()
            extra = 0
            while time.perf_counter() - t_w < args.warmup_seconds and extra < 100000 and not use_dist:
                run_steps(50); extra += 50
                drain(); torch.cuda.synchronize()
            if use_dist:
                # (every rank must run the same number of steps — the collectives are matched —, so the length of the time-based part is agreed on:
                # 1000 steps are timed, the slowest rank's figure decides how many more make up --warmup-seconds)
                t_w = time.perf_counter()
                nw = 64 if args.rehearsal else 1000               # (a rehearsal measures nothing: a short warm-up)
                run_steps(nw); drain(); torch.cuda.synchronize()
                tw = torch.tensor([time.perf_counter() - t_w], dtype=torch.float64, device=device)
                dist.all_reduce(tw, op=dist.ReduceOp.MAX)
                more = int(min(60000.0, max(0.0, args.warmup_seconds - float(tw[0])) / max(float(tw[0]) / nw, 1e-7)))
                more -= more % max(1, pipe["gather"].F)
                if more > 0:
                    run_steps(more); drain(); torch.cuda.synchronize()
            if args.dump_outputs:
                # --dump-outputs: the timed steps start from a restarted accumulation with the per-frame draws from the first, so
                # that their last step computes the same whatever number of steps the time-based warm-up ran (the frame checks
                # replay the passes from here)
                r.rng = GoldenRatioRng()
                r.reset()
                frames_done[0] = 0
                drain()
                torch.cuda.synchronize()
            # R timed blocks of EXACTLY K steps, each bracketed by barrier + synchronize; the MEDIAN block is the one reported.  They follow
            # one untimed block run the same way: the first block after the warm-up ran ~2 % slower than the ones after it on an MI355X
            # (MCM line, K = 20: 1.645-1.660 ms against 1.61-1.62 ms), which a median of five hid and one timed block would not
            blocks = []
            nblocks = max(1, args.repeats) + 1
            r.clear_sample_count()
            r.set_profiling(args.profile_kernel)
            for rep in range(nblocks):
                if use_dist:
                    dist.barrier()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run_steps(args.steps)
                drain()
                torch.cuda.synchronize()
                if use_dist:
                    dist.barrier()
                torch.cuda.synchronize()
                blocks.append(time.perf_counter() - t0)
            if args.dump_outputs and rank == 0:
                res["outputs"] = last_outputs()
            blocks = blocks[1:]                                   # (the untimed block)
            tb = torch.tensor(blocks, dtype=torch.float64, device=device)
            if use_dist:
                dist.all_reduce(tb, op=dist.ReduceOp.MAX)          # per block: the slowest rank
            blocks = [float(x) for x in tb]
            dt = sorted(blocks)[len(blocks) // 2]
            res["dt"] = dt
            res["blocks_ms"] = [b * 1e3 for b in blocks]
            res["kernel_ms"], res["launches"] = r.profile()           # HIP events over ALL blocks, on the kernel's stream
            res["side_kernel_ms"], res["side_launches"] = r.profile_side()   # ... and around the sampled passes' launch on the first side stream
            res["tile_classes"] = r.tile_classes()[:2] if (args.renderer == "mcm" and args.tile_classes) else None
            r.set_profiling(False)
            res["samples_local"] = r.sample_count() / nblocks     # per block (every block runs the same K passes)
            tt = torch.tensor([dt, float(res["samples_local"])], dtype=torch.float64, device=device)
            if use_dist:
                tsum = tt.clone(); dist.all_reduce(tsum, op=dist.ReduceOp.SUM)
                res["dt_max"], res["samples"] = dt, float(tsum[1])
            else:
                res["dt_max"], res["samples"] = dt, float(res["samples_local"])
            ok = None                                    # null: nothing was compared
            if args.check and not use_dist and args.renderer == "mcm":
                ok, res["frame_check_kind"] = single_gpu_frame_check()
            if args.check and use_dist:
                ok = True
            if args.check and use_dist:
                # the gathered frame must hold this rank's own rows unchanged
                rows_np = r.global_rows()
                valid_np = rows_np >= 0
                if use_native[0]:
                    if native.receives():
                        frame = native.frame()                          # [H][W][4] float16 on the host
                        own = r.read(N.BUFFER_RENDER)                   # the buffer the last frame was rendered into
                        ok = bool((frame[rows_np[valid_np]].view(np.uint16) == own[valid_np].view(np.uint16)).all())
                        ok = ok and bool(np.isfinite(frame.astype(np.float32)).all()) and bool((frame[..., 3] == 1).all())
                        # and the whole frame, rendered again UNSHARDED on this GPU with the same per-frame draws, must be
                        # bit-identical to what the ranks produced together (outside the timed region)
                        o2 = {'resolution': (W, H), 'transform': transform, 'rng': GoldenRatioRng(), 'fused': bool(args.fused)}
                        whole = vpt_amd.RendererFactory(args.renderer)(ctx, gvol, camera, None, o2)
                        if args.extinction is not None:
                            whole.extinction = args.extinction
                        if args.renderer == "mcm":                # the same kernel variant as the ranks ran
                            whole.set_option(N.OPTION_FAST_MATH, int(bool(args.fast_math)))
                            whole.set_option(N.OPTION_BOUNDARY_ATLAS, int(bool(args.boundary_atlas)))
                        whole.reset()
                        for _ in range(frames_done[0]):
                            whole.render()
                        same = bool((whole.getTexture().view(np.uint16) == frame.view(np.uint16)).all())
                        whole.destroy()
                        ok = ok and same
                else:
                    frame = pipe["gather"].last_frame()                 # every rank holds the assembled frame
                    rows = torch.as_tensor(rows_np, device=device)
                    valid = rows >= 0
                    ok = bool(torch.equal(frame.index_select(0, rows[valid]), pipe["gather"].last_sent()[valid]))
                    if world > 1 or args.force_dist:
                        # and the same frames rendered UNSHARDED on this GPU must give the gathered frame bit for bit
                        torch.cuda.synchronize()
                        r.set_render_target(0, 0)
                        o2 = {'resolution': (W, H), 'transform': transform, 'rng': GoldenRatioRng(), 'fused': bool(args.fused)}
                        whole = vpt_amd.RendererFactory(args.renderer)(ctx, gvol, camera, None, o2)
                        if args.extinction is not None:
                            whole.extinction = args.extinction
                        if args.renderer == "mcm":
                            whole.set_option(N.OPTION_FAST_MATH, int(bool(args.fast_math)))
                            whole.set_option(N.OPTION_BOUNDARY_ATLAS, int(bool(args.boundary_atlas)))
                        whole.reset()
                        for _ in range(frames_done[0]):
                            whole.render()
                        if pipe["tm"] is not None:                      # display form: the gathered frame is the tone-mapped one
                            tm2 = vpt_amd.ToneMapperFactory('artistic')(ctx, whole, {'resolution': (W, H)})
                            tm2.render()
                            same = bool((tm2.getTexture() == frame.cpu().numpy()).all())
                            tm2.destroy()
                        else:
                            same = bool((whole.getTexture().view(np.uint16) == frame.cpu().numpy().view(np.uint16)).all())
                        whole.destroy()
                        ok = ok and same
            torch.cuda.synchronize()
            res["ok"] = ok
            res["root"] = native.root if use_native[0] else -1
            res["bucket_launches"] = (r.bucket_launches() - launches0) if args.renderer == "mcm" else 0
            return res

        def measure_bucket_form():
            """the torch.distributed pipeline once more with VPT_OPTION_BUCKET_KERNEL: reported beside the line, never as its value"""
            was = use_native[0]
            use_native[0] = False
            r.set_option(N.OPTION_BUCKET_KERNEL, 1); bucket_on[0] = True
            b = measure()
            r.set_option(N.OPTION_BUCKET_KERNEL, 0); bucket_on[0] = False
            use_native[0] = was
            state["bucket_form"] = {
                "ms_per_step": b["dt_max"] / args.steps * 1e3, "value": b["samples"] / b["dt_max"], "frames_per_launch": gather.F,
                "frame_check": b["ok"], "bucket_launches": b["bucket_launches"],
                "what": "the torch.distributed pipeline with VPT_OPTION_BUCKET_KERNEL: the %d frames of a bucket by ONE launch per tile class (photon state in "
                        "registers across the bucket; every frame rendered, written to its slot and gathered; frames bit-identical).  Not the line's "
                        "`value`: the single-GPU line launches once per frame, and so does the pipeline it is compared with" % gather.F}

        def measure_single_gpu_reference():
            """N > 1: what ONE GPU does with the whole frame, measured on rank 0 in this very run (the other ranks wait at the barrier): frame by
            frame (what `value` at N = 1 is) and with the bucket kernels (16 frames per launch) — so that the line carries like-for-like ratios
            for both forms of the pipeline.  Unmeasured on hardware with N > 1 until a multi-GPU node runs this."""
            ref = None
            if rank == 0:
                o2 = {'resolution': (W, H), 'transform': transform, 'rng': GoldenRatioRng(), 'fused': bool(args.fused)}
                whole = vpt_amd.RendererFactory(args.renderer)(ctx, gvol, camera, None, o2)
                whole.set_option(N.OPTION_FAST_MATH, int(bool(args.fast_math)))
                whole.reset()
                t_w = time.perf_counter()
                while time.perf_counter() - t_w < 0.3:
                    for _ in range(50):
                        whole.render()
                    ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(200):
                    whole.render()
                ctx.synchronize()
                frame_by_frame = (time.perf_counter() - t0) / 200
                for _ in range(4):
                    whole.play(16, frames=True)
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(12):
                    whole.play(16, frames=True)
                ctx.synchronize()
                bucket = (time.perf_counter() - t0) / (12 * 16)
                cadence = None
                if args.cadence_form > 0:
                    for _ in range(4):
                        whole.play(args.cadence_form, fused=True)
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(12):
                        whole.play(args.cadence_form, fused=True)
                    ctx.synchronize()
                    cadence = (time.perf_counter() - t0) / (12 * args.cadence_form) * 1e3
                whole.destroy()
                ref = {"frame_by_frame_ms": frame_by_frame * 1e3, "bucket_kernels_16_frames_per_launch_ms": bucket * 1e3,
                       "display_cadence_ms_per_pass": cadence,
                       "what": "the whole %dx%d frame on rank 0's GPU alone, same library and options, measured in this run after the timed regions" % (W, H)}
            if use_dist:
                dist.barrier()
            state["single_gpu"] = ref

        def measure_cadence_form():
            """the frame gathered at a display cadence: D passes per launch on every rank (VPT_PLAY_FUSED: same buffers as D x render()), the D-th frame
            all_gathered; per pass; the gathered frame bit-compared with the same passes unsharded.  Beside the line, never its value."""
            D = int(args.cadence_form)
            drain(); torch.cuda.synchronize()
            g1 = FrameGather(dist, torch, W, H, device, always_collective=bool(args.force_dist), frames_per_gather=1)
            rounds = max(2, (args.steps + D - 1) // D)

            def shown_frames(n):
                for _ in range(n):
                    t_ = g1.acquire()
                    r.set_render_target(t_.data_ptr(), nbytes)
                    r.play(D, fused=True)                       # D passes, one launch per tile class, the last frame into the slot
                    r.join()                                    # both streams in front of the collective
                    g1.commit()
                frames_done[0] += n * D
            shown_frames(4 if args.rehearsal else 16)
            g1.wait_all(); torch.cuda.synchronize()
            blocks = []
            for rep in range(max(1, args.repeats)):
                dist.barrier(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                shown_frames(rounds)
                g1.wait_all(); torch.cuda.synchronize()
                dist.barrier(); torch.cuda.synchronize()
                blocks.append(time.perf_counter() - t0)
            tb = torch.tensor(blocks, dtype=torch.float64, device=device)
            dist.all_reduce(tb, op=dist.ReduceOp.MAX)
            dt = sorted(float(x) for x in tb)[len(blocks) // 2]
            ok = None
            if args.check:
                frame = g1.last_frame()
                r.set_render_target(0, 0)
                o2 = {'resolution': (W, H), 'transform': transform, 'rng': GoldenRatioRng(), 'fused': bool(args.fused)}
                whole = vpt_amd.RendererFactory(args.renderer)(ctx, gvol, camera, None, o2)
                if args.extinction is not None:
                    whole.extinction = args.extinction
                whole.set_option(N.OPTION_FAST_MATH, int(bool(args.fast_math)))
                whole.set_option(N.OPTION_BOUNDARY_ATLAS, int(bool(args.boundary_atlas)))
                whole.reset()
                for _ in range(frames_done[0]):
                    whole.render()
                ok = bool((whole.getTexture().view(np.uint16) == frame.cpu().numpy().view(np.uint16)).all())
                whole.destroy()
            r.set_render_target(0, 0)
            torch.cuda.synchronize()
            state["cadence_form"] = {
                "passes_per_shown_frame": D, "ms_per_pass": dt / (rounds * D) * 1e3, "value": float(W) * H * 8 * rounds * D / dt,
                "bytes_per_pass_and_xgmi_link": int(W * gather.rows * 8 // D), "frame_check": ok,
                "what": "every %d-th frame gathered (RGBA16F all_gather), the passes between accumulate on the owning rank by one launch per tile class "
                        "(VPT_PLAY_FUSED); the gathered frame is checked against the same passes rendered unsharded.  Not the line's `value`: the line "
                        "gathers every pass" % D}

        def measure_display_form():
            """the torch.distributed pipeline gathering the frames as the default tone mapper shows them (RGBA8): beside the line, never its value"""
            was = use_native[0]
            use_native[0] = False
            drain(); torch.cuda.synchronize()
            r.set_render_target(0, 0)
            tm = vpt_amd.ToneMapperFactory('artistic')(ctx, r, {'resolution': (W, H)})
            tm.set_option(N.TONEMAPPER_OPTION_TABLE, N.TONEMAPPER_TABLE_ALWAYS)
            r.render(); frames_done[0] += 1
            tm.render()                                          # builds the table and arms the renderer's frame stores with it
            g8 = FrameGather(dist, torch, W, H, device, always_collective=bool(args.force_dist), frames_per_gather=gather.F, texel='rgba8')
            pipe["gather"], pipe["tm"] = g8, tm
            r.set_option(N.OPTION_BUCKET_KERNEL, 1); bucket_on[0] = True
            b = measure()
            r.set_option(N.OPTION_BUCKET_KERNEL, int(bool(args.bucket_kernel and bucket_capable))); bucket_on[0] = bool(args.bucket_kernel and bucket_capable)
            pipe["gather"], pipe["tm"] = gather, None
            tm.destroy()
            use_native[0] = was
            state["display_form"] = {
                "ms_per_step": b["dt_max"] / args.steps * 1e3, "value": b["samples"] / b["dt_max"], "frames_per_launch": gather.F,
                "frame_check": b["ok"], "bucket_launches": b["bucket_launches"], "bytes_per_frame_and_xgmi_link": int(W * gather.rows * 4),
                "what": "the torch.distributed pipeline gathering every frame AS THE DEFAULT (Artistic) TONE MAPPER SHOWS IT: vpt_renderer_play_into_display — the bucket "
                        "kernels look each texel up in the tone mapper's table and write RGBA8 slots, one all_gather per %d frames moves half the bytes of the "
                        "RGBA16F pipeline (%d instead of %d per frame and link); the gathered frame is checked against render() + toneMapper.render() of the same "
                        "frames unsharded.  Not the line's `value`" % (gather.F, W * gather.rows * 4, W * gather.rows * 8)}

        # N > 1 with the native pipeline: FIRST a complete measurement over torch.distributed's own all_gather (the
        # well-trodden path), so that a result exists whatever the library's RCCL pipeline does on this node; THEN the
        # native pipeline under a deadline.  The line printed is the faster of the two; if the native phase does not
        # finish in time, the first measurement is printed instead and the run ends cleanly.
        results = []
        if use_dist and native is not None and args.safe_first and (world > 1 or args.safe_first > 1):
            use_native[0] = False
            results.append(measure())
            state["fallback"] = results[0]
            if args.bucket_form and bucket_capable and not args.bucket_kernel:
                measure_bucket_form()
            if args.display_form and bucket_capable:
                measure_display_form()
            if args.cadence_form > 0 and bucket_capable:
                measure_cadence_form()
            deadline = threading.Timer(args.native_deadline, _native_gave_up)
            deadline.daemon = True
            deadline.start()
            use_native[0] = True
            results.append(measure())
            deadline.cancel()
            state["fallback"] = None
        else:
            results.append(measure())
            if args.bucket_form and bucket_capable and not args.bucket_kernel and not use_native[0]:
                state["fallback"] = results[0]
                measure_bucket_form()
                state["fallback"] = None
            if args.display_form and bucket_capable and not use_native[0]:
                state["fallback"] = results[0]
                measure_display_form()
                state["fallback"] = None
            if args.cadence_form > 0 and bucket_capable and not use_native[0]:
                state["fallback"] = results[0]
                measure_cadence_form()
                state["fallback"] = None
        if rank == 0 and world == 1 and not use_dist and args.kernels_alone and args.renderer == "mcm" and args.tile_classes and args.fused:
            # after the timed region and its frame check: the two class kernels one after the other on ONE stream, HIP events around the pass and
            # around the MISS-tile kernel alone — what each kernel takes with the chip to itself (roofline.per_kernel)
            try:
                r.set_option(N.OPTION_SPLIT_STREAMS, 1); r.set_option(N.OPTION_TILE_CLASSES, 2)
                for _ in range(100):
                    r.render()
                ctx.synchronize()
                r.set_profiling(1)
                for _ in range(200):
                    r.render()
                ctx.synchronize()
                ms_a, n_a = r.profile(); ms_s, n_s = r.profile_side()
                r.set_profiling(False)
                if n_a and n_s:
                    state["alone"] = {"hit_us": (ms_a / n_a - ms_s / n_s) * 1e3, "miss_us": ms_s / n_s * 1e3,
                                      "how": "alone_us: 200 passes with VPT_OPTION_SPLIT_STREAMS 1 + VPT_OPTION_TILE_CLASSES 2 (HIT kernel, then MISS kernel, one stream), HIP events "
                                             "around the pass minus HIP events around the MISS-tile kernel (the HIT figure carries the gap between the two launches)"}
                r.set_option(N.OPTION_TILE_CLASSES, 1)
                r.set_option(N.OPTION_SPLIT_STREAMS, eff_split)
            except Exception as e:                                  # reporting only
                state["alone"] = None
                print("kernels-alone measurement failed: %r" % (e,), file=sys.stderr)
        if args.full and use_dist and args.renderer == "mcm" and (world > 1 or args.force_dist > 1):
            measure_single_gpu_reference()
        res = min(results, key=lambda x: x["dt_max"])
        if len(results) > 1:
            res["other_pipeline_ms_per_step"] = [x["dt_max"] / args.steps * 1e3 for x in results if x is not res][0]
        stream_gbs = None
        if rank == 0 and args.stream_probe:
            try:
                stream_gbs = ctx.stream_read_rate(4 << 30, 10)      # 4 GiB: far beyond the 256 MB Infinity Cache
            except Exception:                                       # reporting only
                stream_gbs = None
        state["stream_gbs"] = stream_gbs
        line0 = make_line(res) if rank == 0 else None
        if args.dump_outputs and rank == 0:
            names = dump_outputs(res.get("outputs") or {}, args.dump_outputs)
            print("bench.py: --dump-outputs: %s written to %s" % (", ".join(n + ".npy" for n in names) or "nothing", args.dump_outputs), file=sys.stderr)
        matrix = r._matrix()
        other = None
        if rank == 0 and world == 1 and args.other_configs and args.renderer == "mcm":
            # the headline renderer goes first: its side streams would share hardware queues with the configurations measured next
            if native is not None:
                native.destroy(); native = None
            r.destroy(); r = None
            other = other_configs(ctx, gvol, vol, args, W, H, torch)

    ok = res["ok"]
    if rank == 0:
        out = line0
        if world == 1 and args.cpu_baseline and args.renderer == "mcm":
            try:
                out["cpu_baseline"] = cpu_baseline(vol, args, matrix, None)
            except Exception as e:                                      # the baseline is reporting only
                out["cpu_baseline"] = {"value": None, "unit": "volume samples/s", "cores": 0, "kind": "port", "sample": "failed: %r" % (e,)}
            try:
                out["cpu_baseline_js"] = cpu_baseline_js(vol, args, matrix)
            except Exception as e:
                out["cpu_baseline_js"] = {"value": None, "unit": "volume samples/s", "cores": 0, "kind": "port", "sample": "failed: %r" % (e,)}
            out["host_cores"] = len(os.sched_getaffinity(0))
        if other is not None:
            out["other_configs"] = other
        sys.stdout.flush()
        os.dup2(real_stdout, 1)
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)
    if native is not None:
        native.destroy()
    if r is not None:
        r.destroy()
    gvol.destroy(); ctx.destroy()
    if use_dist:
        dist.destroy_process_group()
    watchdog.cancel()
    if ok is False:
        raise SystemExit("frame check failed (N = 1: oracle band; N > 1: gathered frame vs rank-local rows)")


if __name__ == "__main__":
    main()
