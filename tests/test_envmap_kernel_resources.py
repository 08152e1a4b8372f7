"""CPU: the environment-map decode kernel (k_env_decode, vpt_kernels_layout.h) compiles for gfx950 without scratch memory or spills, at
full occupancy: it streams 4 to 16 bytes per texel in and 16 out, and a spill would cost more than the decode."""
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_env_decode_fits_without_scratch():
    usage = resource_usage(["vpt_core"])
    k = {n: u for n, u in usage.items() if "k_env_decode" in n}
    assert len(k) == 1, sorted(k)
    for name, u in k.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("Occupancy", 0) >= 8, (name, u)
