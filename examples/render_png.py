#!/usr/bin/env python3
"""Renders a volume with any renderer / tone mapper through the headless RenderingContext and writes PNG files.

    python examples/render_png.py --renderer mcm --tonemapper artistic --frames 64 --out out.png
    python examples/render_png.py --volume data.bvp ...        (BVP container)   --volume data.raw --dims 256 256 256
    python examples/render_png.py --renderer eam --filter quasicubic ...    (volume filter: linear, nearest or quasicubic)
    python examples/render_png.py --renderer eam --tf colour --gradient sobel --gradient-gain 4 ...   (2-D transfer function: the
                                     gradient magnitude is derived on the device as the volume's second channel)
    python examples/render_png.py --volume ct.raw --dims 512 512 300 --bits 16 --signed --window -200,400 ...   (16-bit samples, placed on the
                                     transfer function's axis by a window derived on the device; --window auto: the 0.5 / 99.5 percentiles)
    python examples/render_png.py --window auto --smooth 1 --reduce 1 --gradient sobel ...   (smoothed, then reduced to half resolution, on the
                                     device, before the gradient is derived)
    python examples/render_png.py --window auto --rank median --rank-passes 2 --gradient sobel ...   (impulse noise removed by a 3 x 3 x 3 median
                                     on the device, edges kept, before the gradient is derived; also erode, dilate, open, close)
    python examples/render_png.py --window auto --rank open --components 96,255 --components-min 64 ...   (island removal on the device: only
                                     connected structures of at least 64 voxels in the codes 96 .. 255 keep their texels; --components-keep 1: the
                                     largest only; --components-label: a row of the 2-D transfer function per structure)
    python examples/render_png.py --window auto --components 96,255 --components-keep 1 --distance 96,255 --distance-within 0,25 ...   (a margin on
                                     the device: the texels within 5 voxels of the largest structure; --distance-seeds rest --distance-within 10,
                                     peels 3 voxels off it (squared distances); --distance-channel 8: the second axis of the 2-D transfer
                                     function is the distance from the structure, 8 rows a voxel)
    python examples/render_png.py --renderer mcm --env sky.hdr --tonemapper aces ...   (a Radiance .hdr environment map lights MCS / MCM)

Without --volume a synthetic 128^3 sphere with lattice noise is used.  PNG encoding is plain zlib (no imaging library)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpt_amd                                                     # noqa: E402
from vpt_amd.synthetic import sphere_volume, colour_tf, GoldenRatioRng   # noqa: E402
from vpt_amd.png import write_png                                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", default="")
    ap.add_argument("--dims", type=int, nargs=3, default=None, help="width height depth of a .raw volume")
    ap.add_argument("--renderer", default="mcm")
    ap.add_argument("--tonemapper", default="artistic")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--extinction", type=float, default=None)
    ap.add_argument("--tf", default="default", choices=["default", "colour"])
    ap.add_argument("--filter", default="linear", choices=["linear", "nearest", "quasicubic"])
    ap.add_argument("--gradient", default=None, choices=["central", "sobel"], help="derive the gradient magnitude as second channel (R8 / R16 volumes)")
    ap.add_argument("--gradient-gain", type=float, default=1.0)
    ap.add_argument("--bits", type=int, default=8, choices=[8, 16, 32], help="sample size of a .raw volume: 8, 16 (little-endian integers) or 32 (float)")
    ap.add_argument("--signed", action="store_true", help="16-bit .raw samples are signed")
    ap.add_argument("--window", default=None, help="LO,HI | range | auto: window the volume's values to the transfer function's axis "
                                                   "(auto: the 0.5 / 99.5 percentiles; the range for a float volume)")
    ap.add_argument("--window-format", default="r8", choices=["r8", "r16"])
    ap.add_argument("--rank", default=None, choices=["median", "erode", "dilate", "open", "close"], metavar="OP",
                    help="median | erode | dilate | open | close over the 3 x 3 x 3 box on the device, behind the window and in front of the smoothing (R8 / R16 volumes)")
    ap.add_argument("--rank-passes", type=int, default=1, metavar="N", help="passes of --rank (1 .. 8)")
    ap.add_argument("--components", default=None, metavar="LO,HI", help="connected components of the codes LO .. HI on the device (R8 / R16 volumes), behind --rank: "
                                                                        "without --components-label everything else becomes 0")
    ap.add_argument("--connectivity", type=int, default=6, choices=[6, 18, 26], help="voxels of a component share faces (6), faces or edges (18), faces, edges or corners (26)")
    ap.add_argument("--components-min", type=int, default=1, metavar="N", help="components of fewer than N voxels are dropped")
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument("--components-keep", type=int, default=None, metavar="N", help="only the N largest components keep their texels (default: all that are not dropped)")
    mode.add_argument("--components-label", action="store_true", help="the second channel is the component's rank (1 = the largest) instead of a gradient")
    ap.add_argument("--distance", default=None, metavar="LO,HI", help="exact squared Euclidean distance d2 of every voxel to the codes LO .. HI on the device (R8 / R16 "
                                                                      "volumes), behind --components: see --distance-within and --distance-channel")
    ap.add_argument("--distance-seeds", default="range", choices=["range", "rest"], help="range: the distance to the codes LO .. HI; rest: the depth inside them")
    how = ap.add_mutually_exclusive_group()
    how.add_argument("--distance-within", default=None, metavar="FROM,TO", help="the texels with FROM <= d2 <= TO keep their codes, everything else becomes 0 "
                                                                                 "(squared voxels; TO may be left out: no upper end); the default is 0,")
    how.add_argument("--distance-channel", type=int, default=None, metavar="STEPS", help="the second channel is the distance, STEPS (1 .. 256) rows of the transfer "
                                                                                       "function a voxel, instead of a gradient")
    grid = ap.add_mutually_exclusive_group()
    grid.add_argument("--resample", default=None, metavar="W,H,D", help="resample the volume to W x H x D texels on the device, behind the window and in front of --rank")
    grid.add_argument("--spacing", default=None, metavar="SX,SY,SZ", help="the voxel spacing: resample the volume to cubic voxels on the device (see --voxel-pitch)")
    ap.add_argument("--voxel-pitch", type=float, default=None, metavar="P", help="edge of the cubic voxels of --spacing (default: the smallest spacing; "
                    "--pitch is the camera's)")
    ap.add_argument("--resample-mode", default="filtered", choices=["filtered", "nearest"], help="filtered: linear interpolation / area average in integers "
                    "(R8, RG8, R16, RG16); nearest: texels are copied (labels and masks, every unpacked format)")
    ap.add_argument("--combine", default=None, metavar="FILE", help="a second volume (.bvp, or raw bytes of the primary's --dims; see --combine-bits) combined with the "
                    "volume on the device: behind --resample and in front of --rank, or ('pair') where --gradient runs")
    ap.add_argument("--combine-op", default="mask", choices=["mask", "min", "max", "absdiff", "blend", "pair"], help="mask: keep the codes where LO <= second <= HI; "
                    "blend: ((WA a + WB b + 128) >> 8) + OFFSET, clamped; pair: the second volume becomes the transfer function's second axis")
    ap.add_argument("--combine-bits", type=int, default=8, choices=[8, 16], help="sample size of a raw --combine file")
    ap.add_argument("--combine-range", default=None, metavar="LO,HI", help="the codes of the second volume that --combine-op mask keeps (default: 1 and above)")
    ap.add_argument("--combine-weights", default=None, metavar="WA,WB,OFFSET", help="the weights (1/256 units, -4096 .. 4096) and the offset of --combine-op blend")
    ap.add_argument("--combine-resample", default=None, choices=["nearest", "filtered"], help="bring a second volume of another size to the volume's grid first "
                    "(nearest for masks and labels)")
    ap.add_argument("--smooth", type=int, default=None, metavar="N", help="binomial 3 x 3 x 3 smoothing passes (1 .. 8) on the device, behind the window (R8 / R16 volumes)")
    ap.add_argument("--reduce", type=int, default=None, metavar="N", help="reduce the volume N times to half its resolution on the device, behind the smoothing")
    ap.add_argument("--yaw", type=float, default=0.6)
    ap.add_argument("--pitch", type=float, default=-0.35)
    ap.add_argument("--env", default="", help="Radiance .hdr environment map (MCS and MCM are lit by it)")
    ap.add_argument("--out", default="frame.png")
    a = ap.parse_args()

    window = a.window
    if window not in (None, 'range', 'auto'):
        lo, hi = (float(x) for x in window.split(','))
        window = [lo, hi]
    components = None
    if a.components is not None:
        lo, hi = (int(x) for x in a.components.split(','))
        components = {'lo': lo, 'hi': hi, 'connectivity': a.connectivity, 'minVoxels': a.components_min,
                      'mode': 'label' if a.components_label else 'keep', 'keep': a.components_keep}
    distance = None
    if a.distance is not None:
        lo, hi = (int(x) for x in a.distance.split(','))
        if a.distance_channel is not None:
            distance = {'lo': lo, 'hi': hi, 'seeds': a.distance_seeds, 'mode': 'channel', 'steps': a.distance_channel}
        else:
            first, _, last = (a.distance_within or '0,').partition(',')
            distance = {'lo': lo, 'hi': hi, 'seeds': a.distance_seeds, 'mode': 'within', 'from': int(first), 'to': int(last) if last.strip() else None}
    resample = None
    if a.resample is not None:
        resample = {'size': [int(x) for x in a.resample.split(',')], 'mode': a.resample_mode}
    elif a.spacing is not None:
        resample = {'spacing': [float(x) for x in a.spacing.split(',')], 'pitch': a.voxel_pitch, 'mode': a.resample_mode}
    combine = None
    if a.combine is not None:
        if a.combine.endswith(".bvp"):
            second = vpt_amd.BVPReader(vpt_amd.FileLoader(a.combine))
        else:
            w, h, d = a.dims
            second = vpt_amd.RAWReader(vpt_amd.FileLoader(a.combine), {'width': w, 'height': h, 'depth': d, 'bits': a.combine_bits})
        combine = {'reader': second, 'op': a.combine_op, 'resample': a.combine_resample}
        if a.combine_op == 'mask':
            lo, _, hi = (a.combine_range or '1,').partition(',')
            combine.update({'lo': int(lo), 'hi': int(hi) if hi.strip() else None})
        elif a.combine_op == 'blend':
            wa, wb, offset = (int(x) for x in (a.combine_weights or '128,128,0').split(','))
            combine.update({'wa': wa, 'wb': wb, 'offset': offset})
    rc = vpt_amd.RenderingContext({'resolution': (a.width, a.height), 'components': components, 'combine': combine, 'distance': distance, 'filter': a.filter, 'rng': GoldenRatioRng(),
                                   'gradient': a.gradient, 'gradientGain': a.gradient_gain,
                                   'window': None if window == 'auto' else window, 'windowFormat': a.window_format,
                                   'rank': a.rank, 'rankPasses': a.rank_passes, 'smooth': a.smooth, 'reduce': a.reduce, 'resample': resample})
    rc.resize(a.width, a.height)
    rc.gl.getExtension('EXT_texture_norm16')                      # 16-bit volumes are taken
    if a.volume.endswith(".bvp"):
        reader = vpt_amd.BVPReader(vpt_amd.FileLoader(a.volume))
    elif a.volume:
        w, h, d = a.dims
        reader = vpt_amd.RAWReader(vpt_amd.FileLoader(a.volume), {'width': w, 'height': h, 'depth': d, 'bits': a.bits, 'signed': a.signed})
    else:
        reader = vpt_amd.RAWReader(sphere_volume(128, noise=48.0), {'width': 128, 'height': 128, 'depth': 128})
    if window == 'auto':
        from vpt_amd.readers import GL_FLOAT, GL_HALF_FLOAT
        floats = reader.readMetadata()['modalities'][0]['type'] in (GL_FLOAT, GL_HALF_FLOAT)
        rc.window = 'range' if floats else {'percentiles': [0.5, 99.5]}
    rc.setVolume(reader)
    if a.env:
        rc.setEnvironmentMap(vpt_amd.read_hdr(a.env))
    # orbit the camera a little so that three faces of the volume are visible
    import math
    from vpt_amd.scene import quat
    q = quat.multiply(quat.create(), quat.setAxisAngle(quat.create(), [0, 1, 0], a.yaw), quat.setAxisAngle(quat.create(), [1, 0, 0], a.pitch))
    rc.camera.transform.localRotation = q
    d = 1.7
    rc.camera.transform.localTranslation = [d * math.sin(a.yaw) * math.cos(a.pitch), -d * math.sin(a.pitch), d * math.cos(a.yaw) * math.cos(a.pitch)]
    rc.chooseRenderer(a.renderer)
    rc.chooseToneMapper(a.tonemapper)
    if a.tf == "colour":
        rc.renderer.setTransferFunction(colour_tf(256, 64 if a.gradient or a.components_label or a.distance_channel is not None or (a.combine and a.combine_op == 'pair') else 1))
    if a.extinction is not None and hasattr(rc.renderer, 'extinction'):
        rc.renderer.extinction = a.extinction
    rc.renderer.reset()
    for _ in range(a.frames):
        rc.render()
    write_png(a.out, rc.getFrame())
    print("wrote %s (%s, %s, %s filter, %d frames, %d volume samples)" % (a.out, a.renderer, a.tonemapper, a.filter, a.frames, rc.renderer.sample_count()))
    rc.destroy()


if __name__ == "__main__":
    main()
