"""GPU: the packed form of MCM's settled MISS-tile pass (VPT_OPTION_SETTLED_MISS = 2, k_mcm_miss_packed).  A settled pass leaves nothing behind
but a direction, and that direction is a function of the pixel and of the last reset's two jitter draws: the packed form stores those two
words (8 B per pixel) instead, stops its last event behind the draws and lets the next pass — or k_mcm_materialize — turn them into the
direction and the photon's start.  Everything a caller can read must equal the same calls with the option at 1 (k_mcm_miss_settled) and at 0
(k_mcm_miss) BIT FOR BIT, in both arithmetic variants, after every pass and across every way of leaving and re-entering the form; the
bit-exact variant also equals the CPU oracle.  Frames of 7 x 5 tiles with partial tiles on both edges (waves without a pixel) and of 3 x 2."""
import numpy as np
import pytest

from vpt_amd import _native as N
from vpt_amd.scene import default_camera
from vpt_amd.synthetic import GoldenRatioRng

from test_gpu_parity import Scene, assert_same_bits, to_frame, MCM_BUFFERS

pytestmark = pytest.mark.gpu

FRAMES = [pytest.param((100, 70), id="100x70"), pytest.param((48, 32), id="48x32")]
WHITE = None
# (0.5 is no byte value: a 1x1 float map.  1 + (e - 1) != e for it: the library settles through its read-back probe)
COLOUR = np.array([[[77 / 255, 31 / 255, 0.5, 1.0]]], dtype=np.float32)
ENVS = [pytest.param(WHITE, id="white"), pytest.param(COLOUR, id="colour")]
frames = pytest.mark.parametrize("frame", FRAMES)
fasts = pytest.mark.parametrize("fast", [1, 0], ids=["fast", "exact"])
envs = pytest.mark.parametrize("env", ENVS)


def camera(w, h):
    cam = default_camera(w / h)
    cam.transform.localTranslation = [0, 0, 3]                  # pulled back: the cube covers the middle tiles only
    return cam


def make(gpu_ctx, oracle, frame, fast, option, env, steps=8):
    w, h = frame
    sc = Scene(gpu_ctx, oracle, 24, w, h, "linear", camera=camera(w, h), noise=35.0)
    r = sc.renderer('mcm')
    r.set_option(N.OPTION_FAST_MATH, fast)
    r.set_option(N.OPTION_SETTLED_MISS, option)
    if env is not None:
        r.setEnvironmentMap(env)
    r.extinction = 4; r.steps = steps; r.anisotropy = 0.2
    return sc, r


def all_buffers(r):
    return [r.read(b) for b in MCM_BUFFERS] + [r.getTexture().copy()]


def run_forms(script, gpu_ctx, oracle, frame, fast, env, options=(2, 0), steps=8):
    """script(r, sc, outs, option) under each option; every output and the sample count equal the first's; returns the settled-pass counts"""
    res = []
    for option in options:
        sc, r = make(gpu_ctx, oracle, frame, fast, option, env, steps)
        outs = []
        script(r, sc, outs, option)
        res.append((outs, r.sample_count(), r.settled_passes()))
        r.destroy(); sc.gvol.destroy()
    outs0, n0, _ = res[0]
    for option, (outs, n, _) in zip(options[1:], res[1:]):
        assert n == n0 and len(outs) == len(outs0)
        for k, (x, y) in enumerate(zip(outs0, outs)):
            assert_same_bits(x, y, "option %d against option %d, output %d" % (options[0], option, k))
    return [s for _, _, s in res]


def both_classes(r):
    hit, miss, _ = r.tile_classes()
    assert hit >= 1 and miss >= 1, (hit, miss)


@frames
@fasts
@envs
@pytest.mark.parametrize("steps", [1, 2, 8])
def test_seven_passes_equal_in_all_three_forms(gpu_ctx, oracle, frame, fast, env, steps):
    def script(r, sc, outs, option):
        r.reset()
        both_classes(r)
        counts = []
        for _ in range(7):
            r.render()
            outs.extend(all_buffers(r))                          # (the read-back materialises: every packed pass starts from the direction array)
            counts.append(r.settled_passes())
        if option:
            assert counts[6] == counts[5] + 1 == counts[4] + 2, counts   # the last two passes took the settled form
        else:
            assert counts[6] == 0
        assert r.tile_classes()[2] == 0

    run_forms(script, gpu_ctx, oracle, frame, fast, env, options=(2, 1, 0), steps=steps)


@frames
@fasts
@envs
def test_packed_passes_in_a_row(gpu_ctx, oracle, frame, fast, env):
    """no read-back between the passes: from the second packed pass on the prologue turns the records into direction and start"""
    def script(r, sc, outs, option):
        r.reset()
        both_classes(r)
        for _ in range(9):
            r.render()
        if option:
            assert r.settled_passes() >= 4
        outs.extend(all_buffers(r))
        outs.extend(all_buffers(r))                              # nothing is owed: a second read changes nothing

    run_forms(script, gpu_ctx, oracle, frame, fast, env, options=(2, 1, 0))


def settle(r, n=6):
    for _ in range(n):
        r.render()


@frames
@fasts
@pytest.mark.parametrize("what", ["read-back", "option", "play", "environment", "camera", "fast-math"])
def test_transitions(gpu_ctx, oracle, frame, fast, what):
    def script(r, sc, outs, option):
        r.reset()
        both_classes(r)
        settle(r)
        before = r.settled_passes()
        if option:
            assert before >= 3                                  # white: settled from the first event on
        if what == "read-back":
            outs.append(r.read(N.BUFFER_MCM_DIRECTION))
            settle(r, 2)
            outs.append(r.read(N.BUFFER_MCM_POSITION))
            settle(r, 2)
        elif what == "option":
            if option:
                r.set_option(N.OPTION_SETTLED_MISS, 1)
            settle(r, 2)
            if option:
                r.set_option(N.OPTION_SETTLED_MISS, 2)
            settle(r, 3)
        elif what == "play":
            r.play(4, frames=True)
            outs.extend(r.read_frame_slot(k).copy() for k in range(4))
            settle(r, 3)
        elif what == "environment":
            r.setEnvironmentMap(COLOUR)                         # the mean moves again: the ordinary kernel until the next reset
            settle(r, 2)
            outs.extend(all_buffers(r))
            r.reset()
            settle(r, 8)                                        # ... and settles through the probe
        elif what == "camera":
            sc.camera.transform.localTranslation = [0.05, 0.02, 2.9]
            settle(r, 2)                                        # another matrix without a reset: the classes are void
            outs.extend(all_buffers(r))
            r.reset()
            both_classes(r)
            settle(r, 4)
        elif what == "fast-math":
            r.set_option(N.OPTION_FAST_MATH, 1 - fast)
            settle(r, 3)
            r.set_option(N.OPTION_FAST_MATH, fast)
            settle(r, 2)
        if option:
            assert r.settled_passes() > before                  # the form was taken again afterwards
        outs.extend(all_buffers(r))

    run_forms(script, gpu_ctx, oracle, frame, fast, WHITE)


@frames
@fasts
def test_verified_classes(gpu_ctx, oracle, frame, fast):
    """VPT_OPTION_VERIFY_TILE_CLASSES through packed passes (the CHECK instantiation): no event of a MISS tile inside the cube"""
    def script(r, sc, outs, option):
        r.set_option(N.OPTION_VERIFY_TILE_CLASSES, 1)
        r.reset()
        both_classes(r)
        settle(r, 5)
        assert r.tile_classes()[2] == 0
        if option:
            assert r.settled_passes() == 4
        outs.extend(all_buffers(r))

    run_forms(script, gpu_ctx, oracle, frame, fast, WHITE)


@frames
def test_bit_exact_band_against_the_oracle(gpu_ctx, oracle, frame):
    w, h = frame
    sc, r = make(gpu_ctx, oracle, frame, 0, 2, WHITE)
    y0 = 0                                                       # the top rows: MISS tiles from edge to edge
    o = oracle.OracleRenderer('mcm', sc.osc, w, h)
    r.reset()
    both_classes(r)
    o.reset(oracle.make_frame(w, h, sc.m, seed=np.float32(GoldenRatioRng()()), y0=y0, y1=y0 + 4))
    for _ in range(7):
        r.render()
        o.integrate(to_frame(oracle, sc, r._u, y0=y0, y1=y0 + 4))
    assert r.settled_passes() == 6
    for b, s in zip(MCM_BUFFERS, o.state):
        assert_same_bits(r.read(b)[y0:y0 + 4], s.reshape(h, w, 4)[y0:y0 + 4], "state buffer %d, rows %d..%d against the oracle" % (b, y0, y0 + 4))
    r.destroy(); sc.gvol.destroy()
