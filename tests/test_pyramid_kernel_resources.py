"""CPU: every instantiation of the pyramid kernels (vpt_volume_pyramid.hip: k_reduce, k_smooth) compiles for gfx950 without scratch memory
or register spills, with at most 64 KiB of LDS per workgroup and an occupancy of at least 2: the conditions of the sibling units
(tests/test_window_kernel_resources.py).  These are conditions, not measurements (DESIGN.md records the figures the compiler reports)."""
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_pyramid_kernels_use_no_scratch_and_share_a_cu():
    usage = resource_usage(["vpt_volume_pyramid"])
    # k_reduce<KIND, CHANNELS, ALIGNED>: KIND in 0 .. 4 (u8, u16, s8, s16, f32), CHANNELS in {1, 2}, ALIGNED in {false, true}
    reduce = {k: v for k, v in usage.items() if re.match(r"_Z8k_reduceILi[0-4]ELi[12]ELb[01]EE", k)}
    assert len(reduce) == 20, sorted(usage)
    # k_smooth<T, ALIGNED>: T in {uint8_t (h), uint16_t (t)}
    smooth = {k: v for k, v in usage.items() if re.match(r"_Z8k_smoothI[ht]Lb[01]EE", k)}
    assert len(smooth) == 4, sorted(usage)
    assert len(usage) == 24, sorted(usage)                       # no kernel of the unit escapes the conditions below
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) <= 64 * 1024, (name, u)
        assert u.get("Occupancy", 0) >= 2, (name, u)
