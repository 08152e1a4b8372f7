"""GPU: the fast-arithmetic MCM kernels (VPT_OPTION_FAST_MATH: mcm_events_fast / mcm_events_fast_early / mcm_events_miss_fast,
sample_hg_fast, photon_start_fast, fast_path_end of vpt_kernels_mcm.h) against their float64 twin (oracle/vpt_oracle.c vpo_mcm_fast64),
event by event, under the fragile / robust rule of DESIGN.md section 3 (tests/fast_twin_cases.py: the cases and the rule;
tests/test_fast_twin.py holds the twin to the contract oracle on the CPU and measures A_REF).

Teacher-forced on the GPU's own trajectories: after the reset (bit-identical to the oracle's) and after every one of PASSES passes the
four state buffers are read, and the twin runs the pass from the state read before it with the uniforms the host sent; every pixel
the twin calls robust must have taken the twin's branch (bounces, samples) and hold every float within A = GPU_FACTOR * A_REF ulps
(+ the value's sensitivity radius).  Every case in two configurations: the library's defaults (tile classes, settled tiles, split
streams: k_mcm_miss and the HIT-tile kernel) and OPTION_TILE_CLASSES = 0 (the general kernel).  The fragile caps hold on these
trajectories as on the oracle's, sample_count() is P * steps * PASSES, and enough default-configuration cases have MISS tiles.

The cases with extinction 0 (1 / 0 = +inf: every free path is infinite, every event leaves the cube) are the ones a NaN distance
would darken: the position a robust out-of-bounds event resets to, and the environment's radiance, are held like everything else."""
import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N

from fast_twin_cases import (A_REF, GPU_FACTOR, BOUNDS, CASES, PASSES, MAX_FRAGILE_CASE, MAX_FRAGILE_OVERALL, CaseStats, case_id, drawn,
                             renderer, reset_frame, frame_of, hold_pass)
from test_gpu_fuzz import same_bits, MCM_BUFFERS

pytestmark = pytest.mark.gpu
A_GPU = GPU_FACTOR * A_REF
assert A_GPU * 2.0 ** -23 <= min(BOUNDS)                 # the slack never exceeds the bounds of tests/test_gpu_fast_math.py
CONFIGS = {"defaults": (), "general": ((N.OPTION_TILE_CLASSES, 0),)}
MIN_CASES_WITH_MISS_TILES = 5
_DONE = {}


def run_case(gpu_ctx, oracle, key, config):
    """the case's PASSES passes on the device in one configuration, each held to the twin; computed once"""
    if (key, config) in _DONE:
        return _DONE[key, config]
    d = drawn(key)
    w, h = d["w"], d["h"]
    osc = oracle.OracleScene(d["vol"], d["filt"], tf=d["tf"], env=d["env"])
    gvol = vpt_amd.Volume.from_array(gpu_ctx, d["vol"], d["filt"])
    r = renderer(gpu_ctx, gvol, d, CONFIGS[config])
    stats = CaseStats(key)
    who = "fast kernels (%s) vs twin," % config
    r.reset()
    o = oracle.OracleRenderer("mcm", osc, w, h)
    o.reset(reset_frame(oracle, d))
    before = [r.read(b).copy() for b in MCM_BUFFERS]
    for b, got, want in zip(MCM_BUFFERS, before, o.state):
        same_bits(got, want.reshape(h, w, 4), "%s %s reset buffer %d (the option does not touch the reset pass)" % (who, case_id(key), b))
    for _ in range(PASSES):
        r.render()
        fr = frame_of(oracle, d, r._u)
        assert fr.steps == d["steps"] and fr.blur == 0.0
        after = [r.read(b).copy() for b in MCM_BUFFERS]
        hold_pass(oracle, osc, fr, before, after, A_GPU, stats)
        before = after
    stats.samples = r.sample_count()
    stats.expected_samples = w * h * d["steps"] * PASSES
    stats.miss_tiles = r.tile_classes()[1]
    r.destroy(); gvol.destroy()
    print(stats.line(who))
    _DONE[key, config] = stats
    return stats


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_fast_kernels_agree_with_the_twin(gpu_ctx, oracle, key, config):
    s = run_case(gpu_ctx, oracle, key, config)
    who = "fast kernels (%s) vs twin," % config
    assert s.bad == 0, (s.line(who), s.first_bad)
    assert s.fragile_share <= MAX_FRAGILE_CASE, s.line(who)
    assert s.samples == s.expected_samples, (s.samples, s.expected_samples)
    if config == "general":
        assert s.miss_tiles == 0


@pytest.mark.parametrize("config", list(CONFIGS))
def test_conditions_over_all_cases(gpu_ctx, oracle, config):
    all_ = [run_case(gpu_ctx, oracle, key, config) for key in CASES]
    events = sum(s.pixel_events for s in all_); fragile = sum(s.fragile for s in all_)
    codes = np.sum([s.codes for s in all_], axis=0)
    with_miss = [case_id(s.key) for s in all_ if s.miss_tiles > 0]
    print("fast kernels (%s) vs twin, all cases: %d pixel-events, %d fragile (%.4f %%), worst case %.3f %%, events null/scatter/out/absorb %s, "
          "A needed %g of %g, MISS tiles in %d cases" % (config, events, fragile, 100.0 * fragile / events, 100 * max(s.fragile_share for s in all_),
                                                        list(codes), max(s.needed for s in all_), A_GPU, len(with_miss)))
    assert sum(s.bad for s in all_) == 0
    assert fragile <= MAX_FRAGILE_OVERALL * events
    if config == "defaults":
        assert len(with_miss) >= MIN_CASES_WITH_MISS_TILES, with_miss
