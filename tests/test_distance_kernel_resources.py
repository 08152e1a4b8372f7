"""CPU: every kernel of the distance-transform unit (vpt_volume_distance.hip) compiles for gfx950 without scratch memory or register
spills, with at most 64 KiB of LDS per workgroup and an occupancy of at least 2: the conditions of the sibling units
(tests/test_components_kernel_resources.py).  These are conditions, not measurements (DESIGN.md records the figures the compiler reports)."""
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_distance_kernels_use_no_scratch_and_share_a_cu():
    usage = resource_usage(["vpt_volume_distance"])
    # k_edt_x<T>: T in {uint8_t (h), uint16_t (t)}
    rows = {k: v for k, v in usage.items() if re.match(r"_Z7k_edt_xI[ht]E", k)}
    assert len(rows) == 2, sorted(usage)
    # k_edt_line<AXIS>: y and z
    lines = {k: v for k, v in usage.items() if re.match(r"_Z10k_edt_lineILi[12]EE", k)}
    assert len(lines) == 2, sorted(usage)
    # the channel emitter: k_pair<T, DistanceChannel> (vpt_volume_field.h), instantiated here
    emit = {k: v for k, v in usage.items() if re.match(r"_Z6k_pairI[ht]15DistanceChannelE", k)}
    assert len(emit) == 2, sorted(usage)
    # the largest finite d2
    plain = {k: v for k, v in usage.items() if re.match(r"_Z\d+k_largestP", k)}
    assert len(plain) == 1, sorted(usage)
    assert len(usage) == 7, sorted(usage)                        # no kernel of the unit escapes the conditions below
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) <= 64 * 1024, (name, u)
        assert u.get("Occupancy", 0) >= 2, (name, u)
    for name, u in list(rows.items()) + list(lines.items()):    # the row and line passes need no LDS
        assert u.get("LDS Size", 0) == 0, (name, u)
