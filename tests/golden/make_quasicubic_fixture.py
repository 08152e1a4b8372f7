#!/usr/bin/env python3
"""Writes tests/golden/quasicubic_r05.json: what THE REFERENCE'S OWN SHADER TEXT computes when its volume is read through the quasi-cubic
filter (VPT_FILTER_QUASI_CUBIC), fragment by fragment.

The reference filters through src/glsl/mixins/quasiCubicSampling.glsl's formula — per axis, in texel space, U = u R + 0.5, F = fract(U),
U' = floor(U) + F F (3 - 2 F), then one texture() at (U' - 0.5) / R — but never calls it, and its text does not compile as written.  So the
shaders are run as make_glsl_fixtures.py runs them (read from the reference tree at generation time, cooked the same way, executed by
oracle/glsl_interp.py) with a volume sampler whose per-axis weight is that formula's: the LINEAR cell i = floor(u - 0.5) and taps, weight
w' = (w w) (3 - 2 w) of the LINEAR weight w, in fp32, byte texels blended as integers and normalised after.
The transfer function, environment and state textures keep their filters.  The fixture holds data only: volumes, transfer functions,
matrices, per-frame uniforms, and the buffers the renderers hold after the last frame of each sequence.

Scenes: the R8 volume of glsl_r04.json seen from outside (MIP, EAM, ISO, Depth, MCM) and a two-channel RG8 volume with the camera inside it
(MIP, EAM, ISO, Depth).  tests/test_gpu_quasicubic.py holds the HIP library to it."""
import argparse
import base64
import ctypes
import ctypes.util
import json
import math
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import numpy as np
from oracle import glsl_interp as G
import make_glsl_fixtures as M

F = np.float32


def qc_weight(w):
    """f' = (f * f) * (3 - 2 f), every operation rounded to fp32"""
    w = F(w)
    return F(F(w * w) * F(F(3.0) - F(F(2.0) * w)))


_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]


class QuasiCubicSampler(G.Sampler):
    """a LINEAR 3-D sampler whose per-axis weight is smoothstep-shaped: the same two taps, the weight through qc_weight.  The filter's own
    arithmetic is the contract's: the cell coordinate s N - 0.5 and every lerp fused, rounded once (libm fmaf)"""

    def _axis(self, coord, n):
        um = F(_libm.fmaf(float(F(coord)), float(n), -0.5))
        if not math.isfinite(float(um)):
            return (0, 0, F(0.0)) if not um > 0 else (n - 1, n - 1, F(0.0))
        fl = F(np.floor(um))
        i0 = int(fl)
        clamp = lambda i: min(max(i, 0), n - 1)
        return clamp(i0), clamp(i0 + 1), qc_weight(um - fl)

    @staticmethod
    def _lerp(a, b, w):
        return F(_libm.fmaf(float(F(w)), float(F(F(b) - F(a))), float(F(a))))


class ByteVolumeSampler(QuasiCubicSampler):
    """R8 / RG8 as the contract filters them: the integer texel values blended, then * fl32(1/255) (255 * fl32(1/255) == 1 exactly)"""
    INV255 = F(0.00392156862745098)

    def sample(self, coord):
        v = super().sample(coord)
        return G.Vec('f', [F(v.c[0] * self.INV255), F(v.c[1] * self.INV255), v.c[2], v.c[3]])


def qc_volume_sampler(vol):
    t = np.zeros(vol.shape[:3] + (4,), np.float32)           # texture(uVolume, p) = (r, g or 0, 0, 1), the channels as integers
    if vol.ndim == 4:
        t[..., :2] = vol.astype(np.float32)
    else:
        t[..., 0] = vol.astype(np.float32)
    t[..., 3] = 1.0
    return ByteVolumeSampler(t, True)


def compact(kind, r, W, H):
    """what tests/test_gpu_quasicubic.py compares, after the last frame of the sequence (whose buffers depend on every earlier one): the
    accumulator in its attachment's own type, or the four MCM state buffers; the RGBA16F image of ISO only, whose render pass samples
    the volume (the others' render passes do not, and the LINEAR fixture covers them)"""
    last = r["frames"][-1]
    dec = lambda b, shape: np.frombuffer(base64.b64decode(b), np.float32).reshape(shape)
    out = {"uniforms_per_frame": r["uniforms_per_frame"]}
    if kind == "mcm":
        out["state_f32"] = last["state"]
        return out
    if kind in ("mip", "eam"):                                  # R8 / RGBA8: the bytes
        out["acc_u8"] = M.b64(np.rint(dec(last["acc"], (H, W) if kind == "mip" else (H, W, 4)) * 255).astype(np.uint8))
    elif kind == "iso":                                         # RGBA16F
        out["acc_f16"] = M.b64(dec(last["acc"], (H, W, 4)).astype(np.float16))
        out["image_f16"] = M.b64(dec(last["image"], (H, W, 4)).astype(np.float16))
    else:                                                       # Depth: R32F
        out["acc_f32"] = last["acc"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--glsl", default="/root/reference/src/glsl")
    ap.add_argument("--out", default=os.path.join(HERE, "quasicubic_r05.json"))
    args = ap.parse_args()
    parts = G.read_parts(args.glsl)
    W, H = 12, 9
    dims = (9, 11, 13)
    vol = M.make_volume(dims, 3)
    tf = M.make_tf(8, 4)
    env = np.random.default_rng(5).integers(40, 256, size=(3, 4, 4), dtype=np.uint8)
    matrix = M.camera_matrix(W / H, 0.55, -0.3, 1.75)
    sc = {"W": W, "H": H, "matrix": matrix, "vol_s": qc_volume_sampler(vol), "tf_s": M.tf_sampler(tf), "env_s": M.env_sampler(env),
          "reset_seed": 0.6180339887}
    seeds = [0.3819660113, 0.7639320225, 0.1458980338]
    plans = {
        "mip": (M.gen_mip, [{"step": 1.0 / 24, "offset": s} for s in seeds[:2]]),
        "eam": (M.gen_eam, [{"step": 1.0 / 20, "offset": s, "extinction": 40.0, "mix": 1.0 / (k + 1)} for k, s in enumerate(seeds[:2])]),
        "iso": (M.gen_iso, [{"steps": 24, "offset": s, "isovalue": 0.25, "light": [0.48, 0.6, 0.64], "gradient_step": 0.02} for s in seeds[:2]]),
        "depth": (M.gen_depth, [{"step": 1.0 / 24, "offset": s, "extinction": 60.0, "threshold": 0.3, "mix": 1.0 / (k + 1)} for k, s in enumerate(seeds[:2])]),
        "mcm": (M.gen_mcm, [{"seed": s, "extinction": 9.0, "anisotropy": g, "max_bounces": 8, "steps": 6} for s, g in zip(seeds, (0.0, 0.35, -0.5))]),
    }
    fixture = {"_what": __doc__.strip().split("\n\n")[0].replace("\n", " "),
               "scene_r8": {"width": W, "height": H, "volume_u8": M.b64(vol), "volume_shape": list(vol.shape), "tf_rgba8": M.b64(tf), "tf_shape": list(tf.shape),
                            "env_rgba8": M.b64(env), "env_shape": list(env.shape), "mvp_inverse_f32": M.b64(matrix), "camera": [0.55, -0.3, 1.75, 1.0],
                            "filter": "quasicubic", "mcm_reset_seed": sc["reset_seed"]},
               "renderers_r8": {}}
    for name, (fn, frames) in plans.items():
        t0 = time.time()
        r = fn(parts, sc, frames)
        r["uniforms_per_frame"] = frames
        fixture["renderers_r8"][name] = compact(name, r, W, H)
        print("r8 %s: %d frames in %.1f s" % (name, len(frames), time.time() - t0), flush=True)
    # the second scene: RG8 (texture(uVolume, p).rg, the transfer function looked up in 2-D), the camera inside the volume looking out with a
    # wide field of view, a 6 x 5 environment map
    vol2 = np.ascontiguousarray(np.stack([vol, M.make_volume(dims, 21)], axis=-1))
    tf2 = np.random.default_rng(22).integers(0, 256, size=(3, 6, 4), dtype=np.uint8)
    tf2[:, 0, 3] = 0
    m2 = M.camera_matrix(W / H, -2.2, 0.5, 0.2, fovy=1.5)
    env2 = np.random.default_rng(31).integers(0, 256, size=(5, 6, 4), dtype=np.uint8)
    sc2 = dict(sc, matrix=m2, vol_s=qc_volume_sampler(vol2), tf_s=M.tf_sampler(tf2), env_s=M.env_sampler(env2))
    fixture["scene_rg8_inside"] = {"width": W, "height": H, "volume_u8": M.b64(vol2), "volume_shape": list(vol2.shape), "tf_rgba8": M.b64(tf2),
                                   "tf_shape": list(tf2.shape), "env_rgba8": M.b64(env2), "env_shape": list(env2.shape), "mvp_inverse_f32": M.b64(m2),
                                   "camera": [-2.2, 0.5, 0.2, 1.5], "filter": "quasicubic", "mcm_reset_seed": sc["reset_seed"]}
    fixture["renderers_rg8_inside"] = {}
    for name, (fn, frames) in plans.items():
        if name == "mcm":                                       # (MCM: the R8 scene's photon histories above)
            continue
        frames = frames[:2]
        t0 = time.time()
        r = fn(parts, sc2, frames)
        r["uniforms_per_frame"] = frames
        fixture["renderers_rg8_inside"][name] = compact(name, r, W, H)
        print("rg8 inside %s: %d frames in %.1f s" % (name, len(frames), time.time() - t0), flush=True)
    with open(args.out, "w") as f:
        json.dump(fixture, f, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
