"""CPU: every instantiation of the window kernels (vpt_volume_window.hip: k_window, k_range, k_code_histogram) compiles for gfx950 without
scratch memory or register spills, with at most 64 KiB of LDS per workgroup and an occupancy of at least 2: the conditions of the sibling
unit (tests/test_gradient_kernel_resources.py).  These are conditions, not measurements (DESIGN.md records the figures the compiler reports)."""
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_window_kernels_use_no_scratch_and_share_a_cu():
    usage = resource_usage(["vpt_volume_window"])
    # k_window<SRC, OUT, ALIGNED>: SRC in 0 .. 4 (u8, u16, s8, s16, f32), OUT in {1, 2} bytes, ALIGNED in {false, true}
    window = {k: v for k, v in usage.items() if re.match(r"_Z8k_windowILi[0-4]ELi[12]ELb[01]EE", k)}
    assert len(window) == 20, sorted(usage)
    rng = {k: v for k, v in usage.items() if re.match(r"_Z7k_rangeILi[0-4]EE", k)}
    assert len(rng) == 5, sorted(usage)
    hist = {k: v for k, v in usage.items() if re.match(r"_Z16k_code_histogramILi[0-3]EE", k)}
    assert len(hist) == 4, sorted(usage)
    assert len(usage) == 29, sorted(usage)                       # no kernel of the unit escapes the conditions below
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) <= 64 * 1024, (name, u)
        assert u.get("Occupancy", 0) >= 2, (name, u)
