"""GPU: what vpt_renderer_profile / vpt_renderer_profile_side count (vpt_renderer_set_profiling) — one launch per timed pass, the frames
of a fused sequence from one pair of events, every n-th pass with set_profiling(n), nothing carried over a new set_profiling — for the
renderer's own passes and for the passes of the gather pipeline; and that gather, renderer and context are destroyed without an error
after timed passes.  (test_gpu_tile_classes.py holds the side stream's count of a 208 x 144 frame and of a frame without MISS tiles.)"""
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.synthetic import colour_tf

from conftest import orbit_camera
from test_gpu_parity import Scene

pytestmark = pytest.mark.gpu

W = H = 128


def far_scene(ctx, oracle, w=W, h=H):
    """a 16^3 volume seen from far enough that the frame has HIT and MISS tiles"""
    return Scene(ctx, oracle, 16, w, h, tf=colour_tf(48, 1), camera=orbit_camera(w / h, 0.7, -0.3, 3.2))


def test_profile_counts_timed_launches(gpu_ctx, oracle):
    sc = far_scene(gpu_ctx, oracle)
    r = sc.renderer('mcm')                                 # the default stream count: HIT tiles on the context's stream, MISS tiles on a side stream
    r.extinction = 5
    r.reset()
    hit, miss, _ = r.tile_classes()
    assert hit > 0 and miss > 0                            # so every pass puts a launch on the side stream

    r.set_profiling(1)
    r.reset()
    for _ in range(3):
        r.render()
    ms, launches = r.profile()
    assert launches == 3 and ms > 0.0
    # (read from the library before the pool of event pairs became one type: 3, a pair per pass around the MISS-tile kernel)
    side_ms, side_launches = r.profile_side()
    assert side_launches == 3 and side_ms > 0.0

    r.set_profiling(1)                                     # the pairs are handed out from the first again: nothing accumulates
    for _ in range(2):
        r.render()
    assert r.profile()[1] == 2
    assert r.profile_side()[1] == 2

    r.set_profiling(2)                                     # every second pass
    for _ in range(4):
        r.render()
    ms, launches = r.profile()
    assert launches == 2 and ms > 0.0
    r.set_profiling(False)
    r.destroy()

    mip = sc.renderer('mip')
    mip.reset()
    mip.set_profiling(1)
    mip.play(4, fused=True)                                # four passes by one launch: one pair of events that stands for four
    ms, launches = mip.profile()
    assert launches == 4 and ms > 0.0
    mip.destroy(); sc.gvol.destroy()


def test_the_gather_pipeline_counts_its_frames_and_everything_is_destroyed_cleanly(oracle):
    from vpt_amd.tiles import RcclFrameGather
    try:
        uid = RcclFrameGather.unique_id()
    except vpt_amd.VptError as e:
        if e.code == N.ERR_UNSUPPORTED:
            pytest.skip("RCCL does not load: %s" % e)
        raise
    ctx = vpt_amd.Context(0)                               # a context of this test's own: it is destroyed here, after what lives in it
    sc = far_scene(ctx, oracle, 64, 64)
    r = sc.renderer('mip', shard=(0, 1, 8))
    r.reset()
    r.set_profiling(1)
    g = RcclFrameGather(r, uid, 0, 1)
    for _ in range(3):
        g.render()
    g.synchronize()
    ms, launches = r.profile()
    assert launches == 3 and ms > 0.0
    L = N.lib()
    assert L.vpt_gather_destroy(g._h) == N.OK
    g._h = None
    assert L.vpt_renderer_destroy(r._h) == N.OK
    r._h = None
    sc.gvol.destroy()
    assert L.vpt_context_destroy(ctx._h) == N.OK
    ctx._h = None
