"""GPU: the barrier-free prologue of the MISS-tile kernels (k_mcm_miss, k_mcm_miss_settled; plain LINEAR one-channel byte volumes).  Each wave
stages the alpha column of the transfer function into its own quarter of the workgroup's LDS (no workgroup barrier), the state texel is the
last load issued and the pixel constants are computed under its flight, and the kernels map workgroups to listed tiles by a mapping of their
own.  Nothing a caller can read may change: every photon-state buffer and the frame are compared, bit for bit, with the tile classes off and
with the settled form off, VPT_OPTION_VERIFY_TILE_CLASSES must count nothing, and the sample counts agree.

Shapes: a 24 x 32 x 40 byte volume, LINEAR; a 72 x 40 image (one partial tile column, one partial tile row) from the default and an off-axis
camera, and a 65 x 17 image (a one-pixel-wide partial tile column and row: most waves of those tiles have no valid lane at all) from the far
camera, where MISS tiles exist at that size; 8 steps, extinction 4, four passes after a reset, read after the FIRST pass (the one that loads
the position array), the second and the fourth (which recompute it).  Transfer functions of width 2 (the default), 3, 64, 65 and 256 with
random RGBA rows: less than a wave's lanes, exactly a wave's, one more, and four rounds of the column's staging.  The executed-and-discarded
sample shows in no buffer, so the column's lookup is probed: vpt_probe_sample_boundary takes its alpha from it."""
import numpy as np
import pytest

from vpt_amd import _native as N

from test_gpu_parity import Scene, assert_same_bits, MCM_BUFFERS
from test_gpu_miss_wave import eye_camera, CAMERAS

pytestmark = pytest.mark.gpu

DIMS = (40, 32, 24)                                          # (nz, ny, nx)
STEPS, PASSES = 8, 4
VIEWS = {"72x40-default": (72, 40, "default"), "72x40-off-axis": (72, 40, "off-axis"), "65x17-far": (65, 17, "default-far")}
WIDTHS = [2, 3, 64, 65, 256]


def random_tf(width):
    """None = the renderer's default (2 x 1); else one row of random RGBA bytes"""
    if width == 2:
        return None
    return np.random.default_rng(100 + width).integers(0, 256, size=(1, width, 4), dtype=np.uint8)


def all_buffers(r):
    return [r.read(b).copy() for b in MCM_BUFFERS] + [r.getTexture().copy()]


class Shared:
    """the scenes and the runs of this module, each computed once"""

    def __init__(self, gpu_ctx, oracle):
        self.gpu_ctx, self.oracle, self.scenes, self.runs = gpu_ctx, oracle, {}, {}

    def scene(self, view):
        if view not in self.scenes:
            w, h, cam = VIEWS[view]
            camera = eye_camera(w / h, CAMERAS[cam]) if CAMERAS[cam] else None
            self.scenes[view] = Scene(self.gpu_ctx, self.oracle, 0, w, h, camera=camera, noise=40.0, dims=DIMS)
        return self.scenes[view]

    def renderer(self, view, fast, width, classes=1, settled=1, verify=0, **opts):
        r = self.scene(view).renderer('mcm', **opts)
        tf = random_tf(width)
        if tf is not None:
            r.setTransferFunction(tf)
        r.set_option(N.OPTION_FAST_MATH, fast)
        r.set_option(N.OPTION_SPLIT_STREAMS, 2)
        r.set_option(N.OPTION_TILE_CLASSES, classes)
        r.set_option(N.OPTION_SETTLED_MISS, settled)
        r.set_option(N.OPTION_VERIFY_TILE_CLASSES, verify)
        r.extinction = 4; r.steps = STEPS
        return r

    def run(self, view, fast, width, classes=1, settled=1, verify=0):
        """([state buffers..., frame] after the first, second and fourth pass, the sample count, the tile counts, the settled passes)"""
        key = (view, fast, width, classes, settled, verify)
        if key not in self.runs:
            r = self.renderer(view, fast, width, classes, settled, verify)
            r.reset()
            outs = []
            for k in range(PASSES):
                r.render()
                if k in (0, 1, 3):
                    outs += all_buffers(r)
            self.runs[key] = (outs, r.sample_count(), r.tile_classes(), r.settled_passes())
            r.destroy()
        return self.runs[key]


@pytest.fixture(scope="module")
def shared(gpu_ctx, oracle):
    s = Shared(gpu_ctx, oracle)
    yield s
    for sc in s.scenes.values():
        sc.gvol.destroy()


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("fast", [0, 1])
@pytest.mark.parametrize("view", list(VIEWS))
def test_prologue_leaves_every_buffer_as_it_was(shared, view, fast, width):
    w, h, _ = VIEWS[view]
    want, count, _, _ = shared.run(view, fast, width, classes=0)
    got, count_on, (hit, miss, violations), settled_passes = shared.run(view, fast, width)
    print("%s fast %d width %d: %d HIT tiles, %d MISS tiles, %d settled passes" % (view, fast, width, hit, miss, settled_passes))
    assert miss > 0 and hit > 0, (hit, miss)
    assert settled_passes > 0                                # the white 1x1 environment is settled from the first event on
    assert count == count_on == w * h * STEPS * PASSES
    for k, (x, y) in enumerate(zip(got, want)):
        assert_same_bits(x, y, "%s fast %d width %d: tile classes on vs off, output %d" % (view, fast, width, k))
    unsettled, count_u, (_, miss_u, _), passes_u = shared.run(view, fast, width, settled=0)
    assert miss_u == miss and passes_u == 0 and count_u == count
    for k, (x, y) in enumerate(zip(got, unsettled)):
        assert_same_bits(x, y, "%s fast %d width %d: settled form on vs off, output %d" % (view, fast, width, k))
    for settled in (1, 0):                                   # the counting forms of both kernels: same buffers, nothing counted
        checked, count_c, (_, miss_c, violations), _ = shared.run(view, fast, width, settled=settled, verify=1)
        assert miss_c == miss and violations == 0 and count_c == count, (view, fast, width, settled, violations)
        for k, (x, y) in enumerate(zip(checked, want)):
            assert_same_bits(x, y, "%s fast %d width %d settled %d: verifying kernels, output %d" % (view, fast, width, settled, k))


@pytest.mark.parametrize("fast", [0, 1])
def test_a_float_environment_that_settles_late(shared, fast):
    """a 1x1 RGBA32F environment whose constant the running mean misses at first (0.0123): k_mcm_miss runs until the library has seen the
    mean stop, then k_mcm_miss_settled — both prologues in one accumulation, against the general kernel on every tile"""
    env = np.array([[[0.0123, 0.1, 0.7, 1.0]]], dtype=np.float32)
    passes = 12

    def run(classes, settled):
        r = shared.renderer("72x40-default", fast, 65, classes=classes, settled=settled)
        r.setEnvironmentMap(env)
        r.steps = 2                                          # (the library probes the mean after each of the first four passes only, and
                                                             # after eight events it has stopped: with one event per pass it gives up)
        r.reset()
        outs = []
        for k in range(passes):
            r.render()
            if k in (0, 5, passes - 1):
                outs += all_buffers(r)
        res = outs, r.sample_count(), r.settled_passes()
        r.destroy()
        return res

    want, count, _ = run(0, 1)
    got, count_on, settled_passes = run(1, 1)
    print("fast %d: %d of %d passes in the settled form" % (fast, settled_passes, passes))
    assert 0 < settled_passes < passes                       # both kernels ran
    assert count == count_on
    for k, (x, y) in enumerate(zip(got, want)):
        assert_same_bits(x, y, "fast %d: float environment, tile classes on vs off, output %d" % (fast, k))
    off, count_off, passes_off = run(1, 0)
    assert passes_off == 0 and count_off == count
    for k, (x, y) in enumerate(zip(off, want)):
        assert_same_bits(x, y, "fast %d: float environment, settled form off, output %d" % (fast, k))


@pytest.mark.parametrize("fast", [0, 1])
def test_a_shard_runs_the_same_prologue(shared, fast):
    """rank 1 of 3, blocks of 8 rows: the shard's rows against the same rows of the unsharded general kernel"""
    view, width = "72x40-default", 3
    want, _, _, _ = shared.run(view, fast, width, classes=0)
    r = shared.renderer(view, fast, width, verify=1, shard=(1, 3, 8))
    r.reset()
    got = []
    for k in range(PASSES):
        r.render()
        if k in (0, 1, 3):
            got += all_buffers(r)
    g = r.global_rows()
    ok = g >= 0
    hit, miss, violations = r.tile_classes()
    assert miss > 0 and violations == 0, (hit, miss, violations)
    for k, (x, y) in enumerate(zip(got, want)):
        assert_same_bits(x[ok], y[g[ok]], "fast %d: rank 1 of 3, output %d" % (fast, k))
    r.destroy()


@pytest.mark.parametrize("width", WIDTHS + [1024, 2048])
def test_the_alpha_column_gives_the_transfer_functions_alpha(shared, width):
    """vpt_probe_sample_boundary looks alpha up in the per-wave column (RGB in the staged pairs): RGBA equal to the brick sampler's, bit for bit.
    Widths 1024 and 2048 (the widest accepted): the probe's image and its four columns pass 64 KiB of dynamic LDS, which the launch asks for"""
    r = shared.renderer("72x40-default", 1, width)
    rng = np.random.default_rng(width)
    n = 4000 + 37                                            # (a last, partial wave and workgroup)
    p = rng.uniform(0.0, 1.0, size=(n, 3))
    axis = rng.integers(0, 3, size=n)
    beyond = np.where(rng.random(n) < 0.2, 1e-6, rng.uniform(0.0, 2.0, size=n) ** 3 + 1e-6)
    p[np.arange(n), axis] = np.where(rng.random(n) < 0.5, 1.0 + beyond, -beyond)
    extra = rng.random((n, 3)) < 0.15                        # further axes out of range: edges and corners
    p = np.where(extra, np.where(rng.random((n, 3)) < 0.5, 1.0 + rng.uniform(1e-6, 3.0, size=(n, 3)), -rng.uniform(1e-6, 3.0, size=(n, 3))), p)
    p = p.astype(np.float32)
    assert (((p < 0) | (p > 1)).any(axis=1)).all()
    got = r.probe_sample_boundary(p)
    assert_same_bits(got, r.probe_sample(p), "width %d: atlas + alpha column vs bricks + staged pairs, %d positions" % (width, n))
    assert_same_bits(got, r.probe_sample(np.clip(p, np.float32(0), np.float32(1))), "width %d: ... at the clamped position" % width)
    r.destroy()
