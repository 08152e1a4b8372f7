"""CPU: every kernel of the resampling unit (vpt_volume_resample.hip) compiles for gfx950 without scratch memory or register spills, with
at most 64 KiB of LDS per workgroup and an occupancy of at least 2: the conditions of the sibling units
(tests/test_distance_kernel_resources.py).  These are conditions, not measurements (DESIGN.md records the figures the compiler reports)."""
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_resample_kernels_use_no_scratch_and_share_a_cu():
    usage = resource_usage(["vpt_volume_resample"])
    # k_resample_x<T, CH>: T in {uint8_t (h), uint16_t (t)}, one and two channels
    rows = {k: v for k, v in usage.items() if re.match(r"_Z12k_resample_xI[ht]Li[12]EE", k)}
    assert len(rows) == 4, sorted(usage)
    # k_resample_yz<T>
    planes = {k: v for k, v in usage.items() if re.match(r"_Z13k_resample_yzI[ht]E", k)}
    assert len(planes) == 2, sorted(usage)
    # k_resample_nearest<BYTES, PER>: one texel a lane for every texel size, one dword a lane for byte and 16-bit texels
    nearest = {k: v for k, v in usage.items() if re.match(r"_Z18k_resample_nearestILi(1ELi1|2ELi1|4ELi1|8ELi1|1ELi4|2ELi2)EE", k)}
    assert len(nearest) == 6, sorted(usage)
    assert len(usage) == 12, sorted(usage)                       # no kernel of the unit escapes the conditions below
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) <= 64 * 1024, (name, u)
        assert u.get("Occupancy", 0) >= 2, (name, u)
    for name, u in list(nearest.items()) + list(planes.items()):      # the gather and the plane pass need no LDS
        assert u.get("LDS Size", 0) == 0, (name, u)
    for name, u in rows.items():                                 # the staged rows: 16 KiB and the dword in front of them
        assert u.get("LDS Size", 0) == 16388, (name, u)
