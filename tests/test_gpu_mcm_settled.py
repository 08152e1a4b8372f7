"""GPU: the settled form of MCM's MISS-tile pass (VPT_OPTION_SETTLED_MISS, k_mcm_miss_settled).  Under a 1x1 environment the running mean of a
MISS tile's pixel stops moving within the first events after a reset; from then on its passes neither read nor write [radiance, samples] and
store no frame texel, and the samples owed are added before anything else reads them.  Everything a caller can read — the four state
buffers, the frame, the sample count — must equal the same run with the option off, BIT FOR BIT, in both arithmetic variants, with the class
kernels on two streams and one after the other on one; the contract variant also equals the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

from vpt_amd import _native as N
from vpt_amd.scene import default_camera
from vpt_amd.synthetic import GoldenRatioRng

from test_gpu_parity import Scene, assert_same_bits, to_frame, env_map, MCM_BUFFERS

pytestmark = pytest.mark.gpu

# frame, volume, steps: 11 x 7 tiles with a cubic volume, 8 x 6 tiles with an odd one
GEOMETRIES = [pytest.param((176, 112, 24, None, 5), id="176x112-24-steps5"), pytest.param((128, 96, 0, (17, 23, 9), 8), id="128x96-17x23x9-steps8")]
# VPT_OPTION_SPLIT_STREAMS 1 runs the class kernels one after the other (VPT_OPTION_TILE_CLASSES 2), 2 side by side (the default)
variants = pytest.mark.parametrize("fast,split", [(0, 2), (1, 2), (0, 1), (1, 1)])
geometries = pytest.mark.parametrize("geom", GEOMETRIES)
COLOUR = np.array([[[77, 200, 31, 255]]], dtype=np.uint8)


def scene(gpu_ctx, oracle, geom, env=None, filt="linear"):
    w, h, n, dims, _ = geom
    return Scene(gpu_ctx, oracle, n, w, h, filt, env=env, camera=default_camera(w / h), noise=35.0, dims=dims)


def renderer(sc, geom, fast, split, settled, **opts):
    r = sc.renderer('mcm', **opts)
    r.set_option(N.OPTION_FAST_MATH, fast)
    r.set_option(N.OPTION_SPLIT_STREAMS, split)
    if split == 1:
        r.set_option(N.OPTION_TILE_CLASSES, 2)
    r.set_option(N.OPTION_SETTLED_MISS, settled)
    r.extinction = 4; r.steps = geom[4]; r.anisotropy = 0.2
    return r


def all_buffers(r):
    return [r.read(b) for b in MCM_BUFFERS] + [r.getTexture().copy()]


def both_classes(r):
    hit, miss, _ = r.tile_classes()
    assert hit > 0 and miss > 0, (hit, miss)


def compare(script, gpu_ctx, oracle, geom, fast, split, env=None, filt="linear", **opts):
    """runs script(r, sc, outs, on) with the option off and on; every output and the sample count equal; returns the on-run's settled passes"""
    res = []
    for settled in (0, 1):
        sc = scene(gpu_ctx, oracle, geom, env, filt)
        r = renderer(sc, geom, fast, split, settled, **opts)
        outs = []
        script(r, sc, outs, bool(settled))
        res.append((outs, r.sample_count(), r.settled_passes()))
        r.destroy(); sc.gvol.destroy()
    (a, na, sa), (b, nb, sb) = res
    assert sa == 0 and na == nb and len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert_same_bits(y, x, "settled MISS tiles on vs off, output %d" % k)
    return sb


def oracle_run(oracle, sc, r, passes, check):
    """the oracle beside r: reset, `passes` render() calls; check(k) after pass k"""
    o = oracle.OracleRenderer('mcm', sc.osc, sc.w, sc.h)
    r.reset()
    o.reset(oracle.make_frame(sc.w, sc.h, sc.m, seed=np.float32(GoldenRatioRng()())))
    for k in range(passes):
        r.render()
        o.render(to_frame(oracle, sc, r._u))
        check(k, o)


@geometries
@variants
@pytest.mark.parametrize("env", [None, COLOUR], ids=["white", "colour"])
def test_plain_accumulation(gpu_ctx, oracle, geom, fast, split, env):
    """reset, six render() calls: the first pass is the ordinary one, five run the settled kernel"""
    steps = geom[4]
    seen = {}

    def script(r, sc, outs, on):
        r.reset()
        both_classes(r)
        for _ in range(6):
            r.render()
        outs.extend(all_buffers(r))
        rad = outs[3].reshape(-1, 4)
        done = rad[:, 3] == steps * 6                           # every event of these pixels deposited the environment (all MISS-tile pixels do)
        assert done.sum() > 256
        colours = np.unique(rad[done][:, :3].view(np.uint32), axis=0)
        assert len(colours) == 1, colours                       # ... and they hold one bit pattern: the environment's constant as the mean keeps it
        want = (np.float32([255, 255, 255]) if env is None else env[0, 0, :3].astype(np.float32)) / np.float32(255)
        assert np.all(np.abs(colours[0].view(np.float32) - want) <= 4 * np.spacing(want)), (colours[0].view(np.float32), want)
        seen[on] = colours[0]
        assert r.tile_classes()[2] == 0

    assert compare(script, gpu_ctx, oracle, geom, fast, split, env) == 5
    assert np.array_equal(seen[True], seen[False])
    if not fast:
        sc = scene(gpu_ctx, oracle, geom, env)
        r = renderer(sc, geom, fast, split, 1)

        def check(k, o):
            if k in (2, 5):                                      # (a read-back in the middle: the samples owed are added first)
                for b, s in zip(MCM_BUFFERS, o.state):
                    assert_same_bits(r.read(b), s.reshape(sc.h, sc.w, 4), "state buffer %d pass %d against the oracle" % (b, k))
            assert_same_bits(r.getTexture(), o.image_f16(), "frame %d against the oracle" % k)

        oracle_run(oracle, sc, r, 6, check)
        assert r.settled_passes() == 5 and r.sample_count() == sc.w * sc.h * steps * 6
        r.destroy(); sc.gvol.destroy()


@geometries
@variants
def test_read_back_in_the_middle(gpu_ctx, oracle, geom, fast, split):
    def script(r, sc, outs, on):
        r.reset()
        both_classes(r)
        for _ in range(3):
            r.render()
        outs.append(r.read(N.BUFFER_MCM_RADIANCE))              # the catch-up runs
        if on:
            assert r.settled_passes() == 2
        for _ in range(3):
            r.render()
        outs.extend(all_buffers(r))
        again = all_buffers(r)                                  # nothing is owed: a third read changes nothing
        for x, y in zip(outs[-5:], again):
            assert_same_bits(y, x, "read twice")
        outs.extend(again)

    assert compare(script, gpu_ctx, oracle, geom, fast, split, COLOUR) == 5


def _frame_ring(r):
    p, n = C.c_void_p(), C.c_size_t()
    N.check(N.lib().vpt_renderer_frame_ring_device(r._h, C.byref(p), C.byref(n)))
    return p.value, n.value


@geometries
@variants
@pytest.mark.parametrize("form", ["hooks", "play", "bucket"])
def test_hooks_and_sequences(gpu_ctx, oracle, geom, fast, split, form):
    """integrate and renderFrame apart (no frame store to leave out: the settled kernel from the second pass on); render() mixed with whole-image
    sequence kernels and frame rings; VPT_OPTION_BUCKET_KERNEL through play_into"""
    def hooks(r, sc, outs, on):
        r.reset()
        both_classes(r)
        for k in range(6):
            r.render()
            if k in (1, 5):
                outs.append(r.getTexture().copy())
        outs.extend(all_buffers(r))
        if on:
            assert r.settled_passes() == 5

    def play(r, sc, outs, on):
        r.reset()
        r.render(); r.render()
        r.play(5, fused=True)
        outs.append(r.getTexture().copy())
        r.play(3, frames=True)
        outs.extend(r.read_frame_slot(k).copy() for k in range(3))
        r.render(); r.render()
        outs.extend(all_buffers(r))
        r.play(9, fused=True)                                   # the passes-in-registers kernel: every tile's whole state
        r.render(); r.render()
        outs.extend(all_buffers(r))
        if on:                                                  # (host logic alone under the white environment: exact, by the stream count)
            assert r.settled_passes() == {2: 10, 1: 5}[split]

    def bucket(r, sc, outs, on):
        r.set_option(N.OPTION_BUCKET_KERNEL, 1)
        r.reset()
        r.render(); r.render()
        r.play(4, frames=True)                                  # allocates the ring
        ring, slot = _frame_ring(r)
        for n in (3, 4, 4):
            r.play_into(n, ring, slot)
            outs.extend(r.read_frame_slot(k).copy() for k in range(n))
        r.set_render_target(0, 0)
        r.render(); r.render()
        outs.extend(all_buffers(r))
        if on:                                                  # (one stream: no bucket kernels, the frames one by one)
            assert r.settled_passes() == {2: 3, 1: 10}[split]

    if form == "hooks":
        compare(hooks, gpu_ctx, oracle, geom, fast, split, fused=False)
    else:
        compare(play if form == "play" else bucket, gpu_ctx, oracle, geom, fast, split)


@geometries
@variants
def test_leaving_and_re_entering(gpu_ctx, oracle, geom, fast, split):
    """steps, the arithmetic variant and the option itself change in mid-accumulation; another matrix and a new environment end the settled
    form until the next reset"""
    steps = geom[4]

    def script(r, sc, outs, on):
        def passes(n, settled_after):
            for _ in range(n):
                r.render()
            outs.extend(all_buffers(r))
            if on:
                assert r.settled_passes() == settled_after, (r.settled_passes(), settled_after)

        r.reset()
        both_classes(r)
        passes(3, 2)
        r.steps = 13 - steps                                    # 5 <-> 8
        passes(2, 4)
        r.set_option(N.OPTION_FAST_MATH, 1 - fast)
        passes(2, 6)
        r.set_option(N.OPTION_FAST_MATH, fast)
        r.steps = steps
        passes(1, 7)
        if on:
            r.set_option(N.OPTION_SETTLED_MISS, 0)
        passes(2, 7)
        if on:
            r.set_option(N.OPTION_SETTLED_MISS, 1)
        passes(2, 9)
        sc.camera.transform.localTranslation = [0.05, 0.02, 1.45]     # another matrix without a reset: the classes are void
        passes(2, 9)
        r.reset()
        both_classes(r)
        passes(3, 11)
        r.setEnvironmentMap(np.array([[[40, 90, 255, 255]]], dtype=np.uint8))   # the mean moves towards the new colour
        passes(2, 11)
        r.setEnvironmentMap(env_map(2, 2))
        passes(2, 11)
        r.reset()
        passes(2, 11)                                           # a 2x2 map: never
        r.setEnvironmentMap(np.array([[[255, 128, 0, 255]]], dtype=np.uint8))
        passes(1, 11)
        r.reset()
        passes(3, 13)

    compare(script, gpu_ctx, oracle, geom, fast, split)


@geometries
@variants
def test_destinations(gpu_ctx, oracle, geom, fast, split):
    """a fused pass takes the settled form only into memory that has received every MISS texel since the reset: fresh zero-filled targets (the
    render buffers of idle renderers), the same target again, a second one, back to the renderer's own buffer, the slots of a bucket"""
    def script(r, sc, outs, on):
        holders = [sc.renderer('mcm') for _ in range(3)]
        targets = [h.render_buffer_device() for h in holders]
        r.reset()
        both_classes(r)
        for _ in range(3):
            r.render()
        if on:
            assert r.settled_passes() == 2
        for t in (0, 0, 1):
            r.set_render_target(*targets[t])
            r.render(); r.join(); sc.ctx.synchronize()
            outs.append(holders[t].getTexture().copy())
            r.render(); r.join(); sc.ctx.synchronize()        # the same memory again, not announced anew
            outs.append(holders[t].getTexture().copy())
        r.set_render_target(0, 0)
        r.render()
        outs.extend(all_buffers(r))
        holders[2].reset(); holders[2].play(3, frames=True)         # a bucket of three slots
        ring, slot = _frame_ring(holders[2])
        for _ in range(3):
            r.play_into(3, ring, slot); r.join(); sc.ctx.synchronize()
            outs.extend(holders[2].read_frame_slot(k).copy() for k in range(3))
        r.set_render_target(0, 0)
        r.render()
        outs.extend(all_buffers(r))
        for h in holders:
            h.destroy()

    assert compare(script, gpu_ctx, oracle, geom, fast, split) >= 3


@geometries
@variants
@pytest.mark.parametrize("what", ["inf", "nan", "map", "no-classes", "nearest"])
def test_refusals(gpu_ctx, oracle, geom, fast, split, what):
    env = None
    if what in ("inf", "nan"):
        env = np.array([[[0.5, np.inf if what == "inf" else np.nan, 0.25, 1.0]]], dtype=np.float32)
    elif what == "map":
        env = env_map(6, 5)

    def script(r, sc, outs, on):
        if what == "no-classes":
            r.set_option(N.OPTION_TILE_CLASSES, 0)
        r.reset()
        for _ in range(4):
            r.render()
        outs.extend(all_buffers(r))
        assert r.settled_passes() == 0

    res = []                                                    # (a float environment has no oracle twin: the scene is built without it)
    for settled in (0, 1):
        sc = scene(gpu_ctx, oracle, geom, env if what == "map" else None, "nearest" if what == "nearest" else "linear")
        r = renderer(sc, geom, fast, split, settled)
        if what in ("inf", "nan"):
            r.setEnvironmentMap(env)
        outs = []
        script(r, sc, outs, bool(settled))
        res.append(outs)
        r.destroy(); sc.gvol.destroy()
    for k, (x, y) in enumerate(zip(*res)):
        assert_same_bits(y, x, "%s: output %d" % (what, k))


@geometries
@variants
@pytest.mark.parametrize("world,rows", [(2, 8), (3, 5)])
def test_sharded_rows(gpu_ctx, oracle, geom, fast, split, world, rows):
    def script(r, sc, outs, on):
        r.reset()
        for _ in range(4):
            r.render()
        outs.extend(all_buffers(r))
        if on and min(r.tile_classes()[:2]) > 0:
            assert r.settled_passes() == 3

    for rank in range(world):
        compare(script, gpu_ctx, oracle, geom, fast, split, shard=(rank, world, rows))


@geometries
@variants
def test_verified_classes(gpu_ctx, oracle, geom, fast, split):
    """VPT_OPTION_VERIFY_TILE_CLASSES with the settled kernel: no event of a MISS tile inside the cube"""
    def script(r, sc, outs, on):
        r.set_option(N.OPTION_VERIFY_TILE_CLASSES, 1)
        r.reset()
        both_classes(r)
        for _ in range(5):
            r.render()
        outs.extend(all_buffers(r))
        assert r.tile_classes()[2] == 0

    assert compare(script, gpu_ctx, oracle, geom, fast, split) == 4


@geometries
@variants
@pytest.mark.parametrize("steps", [1, 2])
def test_a_float_constant_that_settles_late(gpu_ctx, oracle, geom, fast, split, steps):
    """a 1x1 RGBA32F environment whose constant the running mean first misses by many ulps (0.0123: 16) and approaches over several events:
    the library reads one MISS pixel back between passes until the mean has stopped (or gives up); whenever it takes the settled form,
    every buffer and every frame — also those of destinations filled while the mean was still moving — equals the option-off run"""
    env = np.array([[[0.0123, 0.1, 0.7, 1.0]]], dtype=np.float32)

    def script(r, sc, outs, on):
        r.setEnvironmentMap(env)
        r.steps = steps
        holder = sc.renderer('mcm')
        target = holder.render_buffer_device()
        r.reset()
        both_classes(r)
        for k in range(12):
            if k == 2:
                r.set_render_target(*target)                    # filled while the mean may still move ...
            if k == 3:
                r.set_render_target(0, 0)
            if k == 9:
                r.set_render_target(*target)                    # ... announced anew: one ordinary pass first
            r.render()
            if k >= 9:
                r.join(); sc.ctx.synchronize()
                outs.append(holder.getTexture().copy())
            else:
                outs.append(r.getTexture().copy())
        r.set_render_target(0, 0)
        r.render()
        outs.extend(all_buffers(r))
        assert r.settled_passes() <= 11
        holder.destroy()

    compare(script, gpu_ctx, oracle, geom, fast, split)
