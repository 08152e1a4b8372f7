"""CPU: the quasi-cubic instantiations (sampler variant VPT_V_QCUBIC = 256) of the MCM integrate / frame-sequence kernels and of the ray
marchers compile for gfx950 within the budgets of their LINEAR counterparts (variant - 256; tests/test_kernel_resources.py): the three
smoothstep weights must not cost the hot kernels their occupancy or push them into scratch memory."""
import re
import shutil

import pytest

from test_snorm_kernel_resources import resource_usage


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_quasicubic_kernels_fit_the_linear_budgets():
    usage = resource_usage(["vpt_mcm_hit", "vpt_mcm_seq", "vpt_march", "vpt_extra"])
    # MCM integrate, R8: bit-exact and fast-math (272 = QCUBIC | FAST), 32-bit and brick-code tables, hooks and fused
    # (one exception, measured: the HIT kernel sits at the 72-VGPR limit of 7 waves, and its quasi-cubic forms with brick-code tables (> 4 GiB
    # of bricks) and / or fast math and the fused render spill up to three VGPRs there, 8 to 16 bytes of scratch; of R8, the fused fast-math
    # form with brick-code tables)
    hot = {k: v for k, v in usage.items() if re.match(r"_Z15k_mcm_integrateILb[01]ELi(256|257|272|273)EE", k)}
    assert len(hot) == 8, sorted(hot)
    for name, u in hot.items():
        spill_ok = name.startswith("_Z15k_mcm_integrateILb1ELi273E")
        assert u.get("ScratchSize", 0) <= (16 if spill_ok else 0) and u.get("VGPRs Spill", 0) <= (2 if spill_ok else 0), (name, u)
        assert u.get("VGPRs", 999) <= 72 and u.get("Occupancy", 0) >= 7, (name, u)
    multi = {k: v for k, v in usage.items() if k.startswith("_Z11k_mcm_multiILi256E") or k.startswith("_Z11k_mcm_multiILi272E")}
    assert len(multi) == 2, sorted(multi)
    for name, u in multi.items():                # (the LINEAR forms may spill a few registers around their pass loop: the same allowance)
        assert u.get("ScratchSize", 0) <= 64 and u.get("VGPRs", 999) <= 72 and u.get("Occupancy", 0) >= 7, (name, u)
    frames = {k: v for k, v in usage.items() if k.startswith("_Z12k_mcm_framesILi256E") or k.startswith("_Z12k_mcm_framesILi272E")}
    assert len(frames) == 2, sorted(frames)
    for name, u in frames.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs", 999) <= 128 and u.get("Occupancy", 0) >= 4, (name, u)
    # every quasi-cubic instantiation of the marchers, ISO / Depth / LAO / DOS and the MCM kernels holds the occupancy of its LINEAR twin (up
    # to 7 waves; two channels: one wave less, the rule tests/test_snorm_kernel_resources.py holds SNORM to) and,
    # one channel, uses scratch memory only where the twin does (two-channel forms may spill a few bytes as their LINEAR twins do)
    qc = {k: v for k, v in usage.items() if re.search(r"k_(mip|eam|mcs|iso|iso_render|depth|lao|dos_slice|mcm_integrate|mcm_multi)I.*Li(\d+)E", k)
          and int(re.search(r"Li(\d+)E", k[k.index("I"):]).group(1)) & 256}
    assert len(qc) >= 90, len(qc)
    for name, u in qc.items():
        m = re.search(r"Li(\d+)E", name[name.index("I"):])
        start = name.index("I") + m.start()
        v = int(m.group(1))
        twin = name[:start] + "Li%dE" % (v - 256) + name[start + len(m.group(0)):]
        assert twin in usage, (name, twin)
        assert u.get("Occupancy", 0) >= min(usage[twin].get("Occupancy", 0), 7) - (1 if v & 8 else 0), (name, u, usage[twin])
        if not v & 8 and "mcm_multi" not in name:          # (k_mcm_multi: the 64-byte allowance above)
            allowance = 16 if name.startswith("_Z15k_mcm_integrateI") else 0       # (see above)
            assert u.get("ScratchSize", 0) <= usage[twin].get("ScratchSize", 0) + allowance, (name, u, usage[twin])
