"""CPU: the MISS-tile kernels of the plain variants (k_mcm_miss, k_mcm_miss_settled; LINEAR one-channel byte volumes, fast-math and bit-exact,
CHECK off) compiled to gfx950 assembly the way tests/test_kernel_resources.py does it: no scratch, at most 64 VGPRs (8 waves per SIMD), and
no workgroup barrier anywhere in their bodies — each wave stages the transfer function's alpha column for itself and orders it with a
wavefront-scope fence (vpt_kernels_mcm.h miss_wave_start)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# k_mcm_miss<FUSE, V in {0, VPT_V_FAST = 16}, CHECK = false, LATE>, k_mcm_miss_settled<V in {0, 16}, CHECK = false, LATE>
PLAIN = re.compile(r"^(_Z10k_mcm_missILb[01]ELi(?:0|16)ELb0ELb[01]EE|_Z18k_mcm_miss_settledILi(?:0|16)ELb0ELb[01]EE)")


@pytest.fixture(scope="module")
def mcm_unit():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not installed")
    csrc = os.path.join(ROOT, "vpt_amd", "csrc")
    res = subprocess.run(["make", "-C", csrc, "-B", "vpt_mcm.s"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert res.returncode == 0, res.stdout.decode()[-2000:]
    return open(os.path.join(csrc, "vpt_mcm.s")).read(), open(os.path.join(csrc, "vpt_mcm.resources.txt")).read()


def plain_kernels(names):
    got = sorted(n for n in names if PLAIN.match(n))
    # fast-math: LATE on and off; bit-exact: LATE on only (vpt_mcm.hip launch_mcm_classes) — fused or not for k_mcm_miss
    assert len(got) == 2 * 3 + 3, got
    return got


def test_plain_miss_kernels_use_no_scratch_and_at_most_64_vgprs(mcm_unit):
    _, resources = mcm_unit
    usage, cur = {}, None
    for line in resources.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1); usage[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            usage[cur][m.group(1).strip()] = int(m.group(2))
    for name in plain_kernels(usage):
        u = usage[name]
        assert u.get("ScratchSize", 0) == 0 and u.get("VGPRs Spill", 0) == 0 and u.get("SGPRs Spill", 0) == 0, (name, u)
        assert u.get("VGPRs", 999) <= 64 and u.get("Occupancy", 0) >= 8, (name, u)


def test_plain_miss_kernels_have_no_workgroup_barrier(mcm_unit):
    asm, _ = mcm_unit
    bodies, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1); bodies[cur] = []
        elif re.match(r"^\.Lfunc_end\d+:", line):
            cur = None
        elif cur:
            bodies[cur].append(line)
    for name in plain_kernels(bodies):
        body = bodies[name]
        assert any("s_endpgm" in l for l in body), name       # (the body was found whole)
        assert any("ds_write_b64" in l for l in body), name   # the alpha column's pairs are staged by the wave itself
        barriers = [l for l in body if re.search(r"\bs_barrier\b", l)]
        assert not barriers, (name, barriers)
