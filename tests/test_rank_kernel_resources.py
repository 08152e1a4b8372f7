"""CPU: every instantiation of the rank-filter kernels (vpt_volume_rank.hip: k_rank_extreme, k_median) compiles for gfx950 without scratch
memory or register spills, with at most 64 KiB of LDS per workgroup and an occupancy of at least 2: the conditions of the sibling units
(tests/test_pyramid_kernel_resources.py).  These are conditions, not measurements (DESIGN.md records the figures the compiler reports)."""
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_rank_kernels_use_no_scratch_and_share_a_cu():
    usage = resource_usage(["vpt_volume_rank"])
    # k_rank_extreme<T, MAX, ALIGNED>: T in {uint8_t (h), uint16_t (t)}, MAX in {false (erosion), true (dilation)}, ALIGNED in {false, true}
    extreme = {k: v for k, v in usage.items() if re.match(r"_Z14k_rank_extremeI[ht]Lb[01]ELb[01]EE", k)}
    assert len(extreme) == 8, sorted(usage)
    # k_median<T, ALIGNED>
    median = {k: v for k, v in usage.items() if re.match(r"_Z8k_medianI[ht]Lb[01]EE", k)}
    assert len(median) == 4, sorted(usage)
    assert len(usage) == 12, sorted(usage)                       # no kernel of the unit escapes the conditions below
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) <= 64 * 1024, (name, u)
        assert u.get("Occupancy", 0) >= 2, (name, u)
