#!/usr/bin/env python3
"""Extracts the surface of a volume at a level on the device and writes it as a mesh: volume file -> level -> PLY (or STL / OBJ by the
file name's ending).

    python examples/export_surface.py --volume ct.raw --dims 512 512 300 --level 120 --out bone.ply
    python examples/export_surface.py --volume ct.raw --dims 512 512 300 --bits 16 --window -200,400 --level 140 --spacing 0.4 0.4 1.0 --out bone.stl
    python examples/export_surface.py --volume data.bvp --level 128 --out surface.obj

The level is in code units (1 .. 255, or 1 .. 65535 for a 16-bit volume); the surface lies half a code below it.  --window LO,HI brings
signed, float or wide-range samples to R8 codes first, on the device.  --spacing and --origin place the vertices: position = voxel index *
spacing + origin.  Without --volume a synthetic 128^3 sphere with lattice noise is used."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import vpt_amd                                                     # noqa: E402
from vpt_amd.synthetic import sphere_volume                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", default="")
    ap.add_argument("--dims", type=int, nargs=3, default=None, help="width height depth of a .raw volume")
    ap.add_argument("--bits", type=int, default=8, choices=[8, 16, 32], help="sample size of a .raw volume: 8, 16 (little-endian integers) or 32 (float)")
    ap.add_argument("--signed", action="store_true", help="16-bit .raw samples are signed")
    ap.add_argument("--window", default=None, metavar="LO,HI", help="window the volume's values to R8 codes on the device first")
    ap.add_argument("--level", type=int, default=128)
    ap.add_argument("--channel", type=int, default=0, choices=[0, 1])
    ap.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 1.0), metavar=("SX", "SY", "SZ"))
    ap.add_argument("--origin", type=float, nargs=3, default=(0.0, 0.0, 0.0), metavar=("OX", "OY", "OZ"))
    ap.add_argument("--out", default="surface.ply")
    a = ap.parse_args()

    ctx = vpt_amd.Context(0)
    ctx.getExtension('EXT_texture_norm16')                        # 16-bit volumes are taken
    if a.volume.endswith(".bvp"):
        reader = vpt_amd.BVPReader(vpt_amd.FileLoader(a.volume))
    elif a.volume:
        w, h, d = a.dims
        reader = vpt_amd.RAWReader(vpt_amd.FileLoader(a.volume), {'width': w, 'height': h, 'depth': d, 'bits': a.bits, 'signed': a.signed})
    else:
        reader = vpt_amd.RAWReader(sphere_volume(128, noise=48.0), {'width': 128, 'height': 128, 'depth': 128})
    vol = vpt_amd.Volume(ctx, reader)
    vol.load()
    if a.window is not None:
        lo, hi = (float(x) for x in a.window.split(','))
        windowed = vol.window(lo, hi, 'r8')
        vol.destroy()
        vol = windowed
    surface = vol.surface(a.level, a.channel)
    vol.destroy()                                                 # the surface owns what it holds
    info = surface.info
    write = {'.stl': surface.write_stl, '.obj': surface.write_obj}.get(os.path.splitext(a.out)[1].lower(), surface.write_ply)
    write(a.out, a.spacing, a.origin)
    print("wrote %s: %d vertices, %d quads (%d triangles), area %.6g, enclosed volume %.6g; %.3f ms on the device" %
          (a.out, info['vertices'], info['quads'], 2 * info['quads'], surface.area(a.spacing), surface.volume(a.spacing), sum(surface.profile.values())))
    surface.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
