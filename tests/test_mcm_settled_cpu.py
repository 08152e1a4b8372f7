"""CPU: what the settled form of MCM's MISS-tile pass (VPT_OPTION_SETTLED_MISS, k_mcm_miss_settled) rests on.  The oracle: under a 1x1
environment every pixel all of whose events left the cube holds ONE bit pattern in radiance.rgb, from the first pass on and in every later
one.  The compiler: every instantiation of the kernel runs without scratch at 8 waves per SIMD."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from vpt_amd.scene import Transform, Node, default_camera, mvp_inverse_matrix
from vpt_amd.synthetic import sphere_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("colour", [(255, 255, 255, 255), (0, 0, 0, 255), (77, 200, 31, 255), (13, 99, 250, 7)])
def test_radiance_of_environment_only_pixels_is_a_fixed_point(oracle, colour):
    w, h, steps, passes = 128, 96, 8, 4
    osc = oracle.OracleScene(sphere_volume(16), "linear", env=np.array([[colour]], dtype=np.uint8))
    m = mvp_inverse_matrix(default_camera(w / h), Transform(Node()))
    o = oracle.OracleRenderer('mcm', osc, w, h)
    o.reset(oracle.make_frame(w, h, m, seed=0.25))
    pattern = None
    for k in range(1, passes + 1):
        o.render(oracle.make_frame(w, h, m, seed=0.125 * k + 0.03, mcm_steps=steps, extinction=4.0))
        rad = o.state[3].reshape(-1, 4)
        done = rad[:, 3] == steps * k
        assert done.sum() > 0.5 * w * h, (k, done.sum())
        seen = np.unique(rad[done][:, :3].view(np.uint32), axis=0)
        assert len(seen) == 1, (colour, k, seen)
        if pattern is None:
            pattern = seen[0]
        assert np.array_equal(seen[0], pattern), (colour, k, seen[0], pattern)
    want = np.float32(colour[:3]) / np.float32(255)
    assert np.all(np.abs(pattern.view(np.float32) - want) <= 4 * np.spacing(np.maximum(want, np.float32(1e-30))))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc not installed")
def test_settled_kernels_use_no_scratch_and_fit_eight_waves():
    csrc = os.path.join(ROOT, "vpt_amd", "csrc")
    res = subprocess.run(["make", "-C", csrc, "vpt_mcm.s"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert res.returncode == 0, res.stdout.decode()[-2000:]
    usage, cur = {}, None
    for line in open(os.path.join(csrc, "vpt_mcm.resources.txt")):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1); usage[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            usage[cur][m.group(1).strip()] = int(m.group(2))
    # both arithmetic variants (0 | VPT_V_FAST = 16), counting violations or not, the sample consumed late (and, fast-math, also early)
    settled = {k: v for k, v in usage.items() if re.match(r"_Z18k_mcm_miss_settledILi(0|16)ELb[01]ELb[01]EE", k)}
    assert len(settled) == 6, sorted(settled)
    for name, u in settled.items():
        assert u.get("ScratchSize", 1) == 0 and u.get("VGPRs", 999) <= 64 and u.get("Occupancy", 0) >= 8, (name, u)
