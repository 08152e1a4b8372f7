"""CPU: the SNORM instantiations (sampler variant VPT_V_SNORM = 128) of the MCM integrate / frame-sequence kernels and of the ray marchers
compile for gfx950 within the register budgets their UNSIGNED_BYTE counterparts are held to (tests/test_kernel_resources.py): the per-tap
decode must not cost the hot kernels their occupancy or push them into scratch memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def resource_usage(units):
    csrc = os.path.join(ROOT, "vpt_amd", "csrc")
    res = subprocess.run(["make", "-C", csrc, "-B"] + [u + ".s" for u in units], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert res.returncode == 0, res.stdout.decode()[-2000:]
    usage, cur = {}, None
    for u in units:
        for line in open(os.path.join(csrc, u + ".resources.txt")):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = m.group(1); usage[cur] = {}
                continue
            m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
            if m and cur:
                usage[cur][m.group(1).strip()] = int(m.group(2))
    return usage


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_snorm_kernels_fit_the_byte_budgets():
    usage = resource_usage(["vpt_mcm_hit", "vpt_mcm_seq", "vpt_march", "vpt_extra"])
    # MCM integrate, one channel, LINEAR: bit-exact and fast-math (144 = SNORM | FAST), 32-bit and brick-code tables, hooks and fused
    hot = {k: v for k, v in usage.items() if re.match(r"_Z15k_mcm_integrateILb[01]ELi(128|129|144|145)EE", k)}
    assert len(hot) == 8, sorted(hot)
    for name, u in hot.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0, (name, u)
        assert u.get("VGPRs", 999) <= 72 and u.get("Occupancy", 0) >= 7, (name, u)
    multi = {k: v for k, v in usage.items() if k.startswith("_Z11k_mcm_multiILi128E") or k.startswith("_Z11k_mcm_multiILi144E")}
    assert len(multi) == 2, sorted(multi)
    for name, u in multi.items():                # (the byte forms may spill a few registers around their pass loop: the same allowance)
        assert u.get("ScratchSize", 0) <= 64 and u.get("VGPRs", 999) <= 72 and u.get("Occupancy", 0) >= 7, (name, u)
    frames = {k: v for k, v in usage.items() if k.startswith("_Z12k_mcm_framesILi128E") or k.startswith("_Z12k_mcm_framesILi144E")}
    assert len(frames) == 2, sorted(frames)
    for name, u in frames.items():
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs", 999) <= 128 and u.get("Occupancy", 0) >= 4, (name, u)
    # every SNORM instantiation of the marchers and MCM kernels holds at least the occupancy of its byte counterpart (variant - 128)
    # and, one channel, uses no scratch memory
    snorm = {k: v for k, v in usage.items() if re.search(r"k_(mip|eam|mcs|iso|depth|lao|dos_slice|mcm_integrate|mcm_multi)I.*Li(1[3-9]\d)E", k)}
    assert len(snorm) >= 60, len(snorm)
    for name, u in snorm.items():
        m = re.search(r"Li(1[3-9]\d)E", name)
        v = int(m.group(1))
        twin = name[:m.start()] + "Li%dE" % (v - 128) + name[m.end():]
        assert twin in usage, (name, twin)
        assert u.get("Occupancy", 0) >= min(usage[twin].get("Occupancy", 0), 7) - (1 if v & 8 else 0), (name, u, usage[twin])
        if not v & 8 and "mcm_multi" not in name:
            assert u.get("ScratchSize", 0) == 0, (name, u)
