"""GPU: the MISS-tile wave of MCM's tile classes (k_mcm_miss, k_mcm_miss_settled) after its prologue moved ahead of the workgroup barrier and
the face of the boundary atlas became a choice per WAVE (vpt_device.h boundary_cell: any axis that is out of range for every active lane,
tried x, y, z; the per-lane path only when there is none).  Nothing a caller can read may change: every photon-state buffer and the frame
are compared, bit for bit, with the tile classes off and with the settled form off, and VPT_OPTION_VERIFY_TILE_CLASSES must count nothing.

Shapes: a 24 x 32 x 40 byte volume (non-cubic: a swapped axis shows), LINEAR; a 72 x 40 image (one partial tile column, one partial tile
row); 8 steps, four passes after a reset; both arithmetic variants.  Cameras: the default one (MISS tiles left and right of the cube: the
x-uniform path), one looking along +y, one off axis from (1.7, 1.3, 2.0) (lanes of one wave leave past edges and corners: the per-lane path)
— and the first two again from four times as far, where the cube covers one tile row only and the tiles above and below it are MISS tiles
(the y-uniform path; looking along +y the z-uniform one).  The executed-and-discarded sample of a MISS event shows in no buffer, so the face
rule itself is probed: the atlas sampler against the brick sampler at the clamped position, for every pattern of out-of-range axes and signs,
whole waves sharing a pattern and waves that mix them."""
import itertools
import math

import numpy as np
import pytest

from vpt_amd import _native as N

from conftest import orbit_camera
from test_gpu_parity import Scene, assert_same_bits, MCM_BUFFERS

pytestmark = pytest.mark.gpu

W, H, DIMS = 72, 40, (40, 32, 24)            # dims = (nz, ny, nx)


def eye_camera(aspect, eye):
    """a camera at `eye` (world: the cube's centre is the origin) looking at the cube's centre"""
    x, y, z = eye
    d = math.sqrt(x * x + y * y + z * z)
    return orbit_camera(aspect, yaw=math.atan2(x, z), pitch=-math.asin(y / d), dist=d)


CAMERAS = {
    "default": None,                                         # (0, 0, 2) looking along -z
    "along+y": (0.0, -2.0, 0.0),
    "off-axis": (1.7, 1.3, 2.0),
    "default-far": (0.0, 0.0, 8.0),
    "along+y-far": (0.0, -8.0, 0.0),
}


class Shared:
    """the scenes and the runs of this module, each computed once"""

    def __init__(self, gpu_ctx, oracle):
        self.gpu_ctx, self.oracle, self.scenes, self.runs = gpu_ctx, oracle, {}, {}

    def scene(self, cam):
        if cam not in self.scenes:
            camera = eye_camera(W / H, CAMERAS[cam]) if CAMERAS[cam] else None
            self.scenes[cam] = Scene(self.gpu_ctx, self.oracle, 0, W, H, camera=camera, noise=40.0, dims=DIMS)
        return self.scenes[cam]

    def run(self, cam, fast, classes=1, settled=1, verify=0):
        """([state buffers..., frame] after the second and the fourth pass, the tile counts, the settled passes)"""
        key = (cam, fast, classes, settled, verify)
        if key not in self.runs:
            r = self.scene(cam).renderer('mcm')
            r.set_option(N.OPTION_FAST_MATH, fast)
            r.set_option(N.OPTION_SPLIT_STREAMS, 2)
            r.set_option(N.OPTION_TILE_CLASSES, classes)
            r.set_option(N.OPTION_SETTLED_MISS, settled)
            r.set_option(N.OPTION_VERIFY_TILE_CLASSES, verify)
            r.extinction = 4; r.steps = 8
            r.reset()
            outs = []
            for k in range(4):
                r.render()
                if k in (1, 3):                              # (a read materialises the MISS tiles' position / transmittance: once mid-sequence)
                    outs += [r.read(b).copy() for b in MCM_BUFFERS] + [r.getTexture().copy()]
            assert r.sample_count() == W * H * 8 * 4
            self.runs[key] = (outs, r.tile_classes(), r.settled_passes())
            r.destroy()
        return self.runs[key]


@pytest.fixture(scope="module")
def shared(gpu_ctx, oracle):
    s = Shared(gpu_ctx, oracle)
    yield s
    for sc in s.scenes.values():
        sc.gvol.destroy()


@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("cam", list(CAMERAS))
def test_miss_wave_leaves_every_buffer_as_it_was(shared, cam, fast):
    want, _, _ = shared.run(cam, fast, classes=0)
    got, (hit, miss, violations), settled_passes = shared.run(cam, fast)
    print("%s fast %d: %d HIT tiles, %d MISS tiles, %d settled passes" % (cam, fast, hit, miss, settled_passes))
    assert miss > 0 and hit > 0, (hit, miss)
    assert settled_passes > 0                                # the white 1x1 environment is settled from the first event on
    for k, (x, y) in enumerate(zip(got, want)):
        assert_same_bits(x, y, "%s fast %d: tile classes on vs off, output %d" % (cam, fast, k))
    unsettled, (_, miss_u, _), passes_u = shared.run(cam, fast, settled=0)
    assert miss_u == miss and passes_u == 0
    for k, (x, y) in enumerate(zip(got, unsettled)):
        assert_same_bits(x, y, "%s fast %d: settled form on vs off, output %d" % (cam, fast, k))
    for settled in (1, 0):                                   # the counting forms of both kernels: same buffers, nothing counted
        checked, (_, miss_c, violations), _ = shared.run(cam, fast, settled=settled, verify=1)
        assert miss_c == miss and violations == 0, (cam, fast, settled, violations)
        for k, (x, y) in enumerate(zip(checked, want)):
            assert_same_bits(x, y, "%s fast %d settled %d: verifying kernels, output %d" % (cam, fast, settled, k))


def out_of_range_patterns():
    """every non-empty set of out-of-range axes in every sign combination: 6 + 12 + 8 patterns of (-1 below 0 | 0 in range | +1 above 1)"""
    return [p for p in itertools.product((-1, 0, 1), repeat=3) if any(p)]


def positions(rng, patterns):
    """one position per pattern row: in-range coordinates anywhere in [0, 1] (texel centres, cell borders and the faces' own edges
    included), out-of-range ones a hair to far beyond the face"""
    patterns = np.asarray(patterns)
    n = len(patterns)
    inside = rng.uniform(0.0, 1.0, size=(n, 3))
    special = rng.choice([0.0, 1.0, 0.5 / 24, 1 - 0.5 / 32, 0.5, 1.5 / 40], size=(n, 3))
    inside = np.where(rng.random((n, 3)) < 0.25, special, inside)
    beyond = np.where(rng.random((n, 3)) < 0.2, 1e-6, rng.uniform(0.0, 3.0, size=(n, 3)) ** 3)
    beyond = np.maximum(beyond, 1e-6)
    p = np.where(patterns == 0, inside, np.where(patterns > 0, 1.0 + beyond, -beyond))
    return p.astype(np.float32)


def test_the_face_rule_gives_the_brick_sample_whatever_the_wave_shares(shared):
    sc = shared.scene("default")
    r = sc.renderer('mcm')
    rng = np.random.default_rng(11)
    pats = out_of_range_patterns()
    assert len(pats) == 26
    rows = []
    for p in pats:                                           # whole waves (64 consecutive positions) sharing one pattern
        rows += [p] * 64
    for axis in range(3):                                    # whole waves sharing ONE out-of-range axis, the other two mixed per lane
        for sign in (-1, 1):
            for _ in range(3):
                w = rng.integers(-1, 2, size=(64, 3))
                w[:, axis] = sign
                rows += [tuple(x) for x in w]
    for _ in range(40):                                      # the patterns mixed inside a wave: no axis shared (the per-lane path), or by chance
        rows += [pats[i] for i in rng.integers(0, len(pats), size=64)]
    rows += [pats[i] for i in rng.integers(0, len(pats), size=37)]      # a last, partial wave
    p = positions(rng, rows)
    assert (((p < 0) | (p > 1)).any(axis=1)).all()
    for a in (0, 1, 2):                                      # the patterns are what they claim to be
        assert ((p[:, a] > 1).astype(int) - (p[:, a] < 0).astype(int) == np.asarray(rows)[:, a]).all()
    got = r.probe_sample_boundary(p)
    want = r.probe_sample(np.clip(p, np.float32(0), np.float32(1)))
    assert_same_bits(got, want, "atlas (face chosen per wave) vs bricks at the clamped position, %d positions" % len(p))
    assert_same_bits(got, r.probe_sample(p), "atlas vs bricks at the position itself")
    r.destroy()
