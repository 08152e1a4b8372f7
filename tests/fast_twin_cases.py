"""The cases and the comparison rule shared by tests/test_fast_twin.py (CPU: the float64 twin of the MCM fast-arithmetic variant against
the contract oracle) and tests/test_gpu_fast_twin.py (GPU: the fast kernels against the twin); the rule is DESIGN.md section 3's.

Cases: random_case / random_camera of tests/test_gpu_fuzz.py for seeds 0..39, then that file's MCM draws of extinction {0, 1, 7, 80},
anisotropy {0, 0.9, -0.7, 1e-6} and bounces {0, 1, 8}, drawn in that order right behind the camera (extinction 0: EXTINCTION_0_SEEDS).
run_random_scene draws fused passes, the first seed and a row shard from the generator before them; here fused = seed odd, first
seed = 1 + seed, no shard, so that the three parameters are a function of the seed alone.  Then three hand-made scenes: a quasi-cubic
volume; a NEAREST volume, seen through a negated projection matrix; a float environment map.  Every case runs PASSES passes of
one event per pixel, every fourth seed of three chained events, TEACHER-FORCED: each pass is compared from the state the side under test
itself had before it, so no error accumulates and every event of a trajectory is checked.

The rule, for `slack` = A ulps (of 2^-23): on every pixel the twin does not call fragile, bounces and samples (through which the branch
taken shows) equal the twin's exactly, an infinite twin value is met exactly, and every other float lies within
min(A * 2^-23, bound) * max(1, |value|) + the value's sensitivity radius, bound = 1e-4 for position and direction and 1e-5 for
transmittance and radiance (the bounds of tests/test_gpu_fast_math.py)."""
import numpy as np

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.scene import Node, Transform, PerspectiveCamera, mvp_inverse_matrix
from vpt_amd.synthetic import GoldenRatioRng

from conftest import orbit_camera
from test_gpu_fuzz import random_case, random_camera

# A_REF: the slack at which the contract oracle (float32, software log / sin / cos / rcp / rsq within 2 ulp) meets the twin on every robust
# pixel-event of the cases below, measured by tests/test_fast_twin.py on the grid of powers of two (it fails at half of it)
A_REF = 8.0
GPU_FACTOR = 8.0                 # the hardware instructions are 1-ulp class and the fast forms chain a few more roundings
BOUNDS = (1e-4, 1e-4, 1e-5, 1e-5)
PASSES = 10
SEEDS = range(40)
EXTINCTION_0_SEEDS = (0, 5, 12, 14, 18, 19, 20, 21, 24, 27, 28)
SCENES = ("quasicubic", "nearest", "float_env")
CASES = [("seed", s) for s in SEEDS] + [("scene", n) for n in SCENES]
MAX_FRAGILE_CASE, MAX_FRAGILE_OVERALL, MIN_EVENTS_PER_CODE = 0.01, 0.001, 10000


class NegatedPerspective(PerspectiveCamera):
    """the same projective map with the homogeneous sign flipped: every unprojected point has w < 0, which the contract divides away and
    the fast variant's normalize(to.xyz - to.w * from) form has to undo with its sign(to.w)"""

    @property
    def projectionMatrix(self):
        m = super().projectionMatrix
        for i in range(16):
            m[i] = -m[i]
        return m


def case_id(key):
    return "%s-%s" % key


def drawn(key):
    """the scene, camera and MCM parameters of a case"""
    kind, which = key
    if kind == "seed":
        rng, vol, (w, h), tf, env, filt, model = random_case(which)
        camera = random_camera(rng, w / h)
        ext = float(rng.choice([0.0, 1.0, 7.0, 80.0])); g = float(rng.choice([0.0, 0.0, 0.9, -0.7, 1e-6])); bounces = int(rng.choice([0, 1, 8]))
        fused, start = bool(which % 2), 1 + which
        steps = 3 if which % 4 == 3 else 1
    else:
        n = SCENES.index(which)
        rng = np.random.default_rng(900 + n)
        vol = rng.integers(0, 256, size=(19, 23, 29), dtype=np.uint8)
        w, h = 96, 64
        tf = rng.integers(0, 256, size=(1, 32, 4), dtype=np.uint8)
        env = (rng.uniform(0, 8, size=(5, 8, 4)).astype(np.float32) if which == "float_env" else None)
        if env is not None:
            env[..., 3] = 1.0
        filt = {"quasicubic": "quasicubic", "nearest": "nearest"}.get(which, "linear")
        model = Transform(Node())
        camera = orbit_camera(w / h)
        if which == "nearest":                           # (and this scene's matrix is the negated one)
            lens = camera.getComponent(PerspectiveCamera)
            camera.components[camera.components.index(lens)] = NegatedPerspective(camera, {'fovy': lens.fovy, 'aspect': lens.aspect, 'near': lens.near, 'far': lens.far})
        fused, start = False, 1
        ext, g, bounces = (7.0, 0.9, 8) if which == "quasicubic" else (80.0, -0.7, 8) if which == "nearest" else (1.0, 0.0, 1)
        steps = 3 if which == "float_env" else 1
    return dict(vol=vol, w=w, h=h, tf=tf, env=env, filt=filt, model=model, camera=camera, fused=fused, start=start,
                extinction=ext, anisotropy=g, bounces=bounces, steps=steps)


def renderer(ctx, gvol, d, options=()):
    """the MCM renderer of a drawn case with the fast-arithmetic variant selected; ctx of test_gpu_fuzz.oracle_only(): no device behind it"""
    r = vpt_amd.RendererFactory("mcm")(ctx, gvol, d["camera"], d["env"],
                                       {'resolution': (d["w"], d["h"]), 'transform': d["model"], 'rng': GoldenRatioRng(d["start"]), 'fused': d["fused"]})
    r.set_option(N.OPTION_FAST_MATH, 1)
    for opt, val in options:
        r.set_option(opt, val)
    if d["tf"] is not None:
        r.setTransferFunction(d["tf"])
    r.extinction = d["extinction"]; r.anisotropy = d["anisotropy"]; r.bounces = d["bounces"]; r.steps = d["steps"]
    return r


def reset_frame(oracle, d):
    m = mvp_inverse_matrix(d["camera"], d["model"])
    return oracle.make_frame(d["w"], d["h"], m, seed=np.float32(GoldenRatioRng(d["start"])()))      # MCMRenderer.js:93: the reset's own draw


def frame_of(oracle, d, u):
    """the oracle's frame of the uniforms the host actually sent"""
    fr = oracle.make_frame(d["w"], d["h"], np.array(list(u.mvp_inverse), np.float32), nthreads=4)
    fr.seed = u.rand_seed; fr.extinction = u.extinction; fr.anisotropy = u.anisotropy; fr.max_bounces = u.max_bounces; fr.steps = u.steps
    fr.blur = u.blur
    return fr


def disagreements(twin, got, slack):
    """the pixels the twin calls robust on which the four state arrays `got` break the rule -> boolean [pixels]"""
    g = np.stack([np.asarray(b, np.float32).reshape(-1, 4) for b in got], axis=1).astype(np.float64)     # [pixel][buffer][4]
    want = twin.state
    ok = (g[:, 1, 3] == want[:, 12]) & (g[:, 3, 3] == want[:, 13])
    with np.errstate(invalid="ignore"):
        for b in range(4):
            v = want[:, 3 * b:3 * b + 3]; x = g[:, b, :3]
            tol = min(slack * 2.0 ** -23, BOUNDS[b]) * np.maximum(1.0, np.abs(v)) + twin.radius[:, b:b + 1]
            ok &= np.where(np.isfinite(v), np.abs(x - v) <= tol, x == v).all(axis=1)
    return (twin.fragile == 0) & ~ok


class CaseStats:
    def __init__(self, key):
        self.key, self.pixel_events, self.fragile, self.bad, self.needed = key, 0, 0, 0, 0.0
        self.codes = np.zeros(4, np.int64)
        self.first_bad = None

    @property
    def fragile_share(self):
        return self.fragile / max(self.pixel_events, 1)

    def line(self, who):
        return "%s %s: %d pixel-events, %d fragile (%.4f %%), %d robust disagreements, A needed %g, events null/scatter/out/absorb %s" % (
            who, case_id(self.key), self.pixel_events, self.fragile, 100 * self.fragile_share, self.bad, self.needed, list(self.codes))


def hold_pass(oracle, osc, fr, before, after, top, stats):
    """one teacher-forced pass: the twin from `before` at slack `top` against `after`; the smallest slack of the grid top/8 .. top (powers
    of two) at which every robust pixel agrees is recorded as the slack the pass needs"""
    twin = oracle.mcm_fast64(osc, fr, before, top)
    bad = disagreements(twin, after, top)
    stats.pixel_events += twin.fragile.size * fr.steps
    stats.fragile += int(twin.fragile.sum()) * fr.steps
    stats.codes += np.bincount(twin.codes.reshape(-1), minlength=4)[:4]
    stats.bad += int(bad.sum())
    if bad.any() and stats.first_bad is None:
        k = int(np.nonzero(bad)[0][0])
        stats.first_bad = "pixel %d: twin %s radius %s codes %s, got %s" % (
            k, twin.state[k].tolist(), twin.radius[k].tolist(), twin.codes[k].tolist(), [np.asarray(b).reshape(-1, 4)[k].tolist() for b in after])
    needed = top if not bad.any() else 2 * top
    for a in (top / 8, top / 4, top / 2):
        if bad.any():
            break
        if not disagreements(oracle.mcm_fast64(osc, fr, before, a), after, a).any():
            needed = a
            break
    stats.needed = max(stats.needed, needed)
    return twin
