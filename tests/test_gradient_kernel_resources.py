"""CPU: every instantiation of the volume-operation kernels (vpt_volume_ops.hip: k_gradient, k_histogram, k_histogram_rg, k_read_block)
compiles for gfx950 without scratch memory or register spills, and with at most 64 KiB of LDS per workgroup, so that at least two
workgroups share a CU.  These are conditions, not measurements (DESIGN.md records the figures the compiler reports)."""
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_volume_operation_kernels_use_no_scratch_and_share_a_cu():
    usage = resource_usage(["vpt_volume_ops"])
    # k_gradient<T, OP, ALIGNED>: T in {uint8_t (h), uint16_t (t)}, OP in {0, 1}, ALIGNED in {false, true}
    grad = {k: v for k, v in usage.items() if re.match(r"_Z10k_gradientI[ht]Li[01]ELb[01]EE", k)}
    assert len(grad) == 8, sorted(usage)
    hist = {k: v for k, v in usage.items() if re.match(r"_Z1[14]k_histogram(_rg)?I[ht]E", k)}
    assert len(hist) == 4, sorted(usage)
    read = {k: v for k, v in usage.items() if k.startswith("_Z12k_read_block")}
    assert len(read) == 1, sorted(usage)
    assert len(usage) == 13, sorted(usage)                       # no kernel of the unit escapes the conditions below
    for name, u in usage.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("LDS Size", 0) <= 64 * 1024, (name, u)
        assert u.get("Occupancy", 0) >= 2, (name, u)             # two 256-thread workgroups per CU = 2 waves per SIMD
