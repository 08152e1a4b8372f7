"""CPU: the 16-bit normalised instantiations (sampler variant VPT_V_NORM16 = 512, | VPT_V_SNORM = 640) of the MCM integrate / frame-sequence
kernels, the ray marchers, ISO / Depth / LAO / DOS and the probes compile for gfx950 within the budgets of the byte and R32F forms
(tests/test_kernel_resources.py): the per-tap decode of two-byte texels must not cost the hot kernels their occupancy or push them into
scratch memory."""
import os
import re
import shutil

import pytest

from test_snorm_kernel_resources import ROOT, resource_usage


def variant(name):
    """the template argument that carries VPT_V_NORM16 (k_mip<mode, V>: the second one), or (None, 0)"""
    for m in re.finditer(r"Li(\d+)E", name[name.index("I"):]):
        if int(m.group(1)) & 512:
            return m, int(m.group(1))
    return None, 0


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_norm16_kernels_fit_the_budgets():
    usage = resource_usage(["vpt_mcm_hit", "vpt_mcm_seq", "vpt_mcm", "vpt_march", "vpt_extra", "vpt_core"])
    # MCM integrate, one channel, LINEAR: bit-exact and fast-math, 32-bit and brick-code tables, hooks and fused; UNORM and SNORM
    hot = {k: v for k, v in usage.items() if re.match(r"_Z15k_mcm_integrateILb[01]ELi(512|513|528|529|640|641|656|657)EE", k)}
    assert len(hot) == 16, sorted(hot)
    for name, u in hot.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (name, u)
        assert u.get("VGPRs", 999) <= 72 and u.get("Occupancy", 0) >= 7, (name, u)
    frames = {k: v for k, v in usage.items() if re.match(r"_Z12k_mcm_framesILi(512|528|640|656)E", k)}
    assert len(frames) == 4, sorted(frames)
    for name, u in frames.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs", 999) <= 128 and u.get("Occupancy", 0) >= 4, (name, u)
    # every other 16-bit instantiation against its R32F twin (the same bits with VPT_V_F32 for VPT_V_NORM16 | VPT_V_SNORM): at least the twin's
    # occupancy (two channels: one wave less, the rule the SNORM and quasi-cubic budgets hold), and one channel no scratch memory, except
    # where the twin's own form has some: k_mcm_multi (the 64-byte allowance of tests/test_kernel_resources.py) and the fused quasi-cubic
    # MCM integrate forms (up to 16 bytes, as tests/test_quasicubic_kernel_resources.py allows their R8 twins).
    # A kernel compiled FOR a number of waves (k_mip: VPT_MIP_WAVES, the measured choice of vpt_kernels.h) is held to that number where
    # its twin happens to come out above it: inside the budget the allocator is free.  The R32F forms moved by a wave in both directions
    # when their sampler learnt GL's index clamp (the fused k_mip<1, 36 | 292>: 73 / 74 VGPRs -> 69 / 70); the 16-bit forms, whose
    # code did not change, stay at 74.
    kernels = {k: v for k, v in usage.items()
               if re.search(r"k_(mip|eam|mcs|iso|iso_render|depth|lao|dos_slice|mcm_integrate|mcm_multi|probe_sample|probe_sample_boundary)I", k)
               and variant(k)[1]}
    assert len(kernels) >= 500, len(kernels)
    mip_waves = int(re.search(r"#define VPT_MIP_WAVES (\d+)", open(os.path.join(ROOT, "vpt_amd", "csrc", "vpt_kernels.h")).read()).group(1))
    assert 6 <= mip_waves <= 8
    for name, u in kernels.items():
        m, v = variant(name)
        start = name.index("I") + m.start()
        # (LAO and EAM with brick-code tables take the unaligned 16-bit loads where their R32F twins take VPT_V_ALIGNED = 4)
        twins = [name[:start] + "Li%dE" % (((v & ~(512 | 128)) | 32) | a) + name[start + len(m.group(0)):] for a in (0, 4)]
        twin = next((t for t in twins if t in usage), None)
        assert twin is not None, (name, twins)
        t = usage[twin]
        budget = mip_waves if "k_mipI" in name else 7
        assert u.get("Occupancy", 0) >= min(t.get("Occupancy", 0), 7, budget) - (1 if v & 8 else 0), (name, u, t)
        if not v & 8:
            if "mcm_multi" in name:
                allowance = 64
            elif name.startswith("_Z15k_mcm_integrateILb1") and v & 256:
                allowance = 16
            else:
                allowance = 0
            assert u.get("ScratchSize", 0) <= allowance, (name, u, t)
    # no k_mcm_miss of their own: the MISS tiles of a 16-bit volume run the FLOAT one (vpt_mcm.hip launch_mcm_classes)
    assert not [k for k in usage if k.startswith("_Z10k_mcm_missI") and variant(k)[1]]
