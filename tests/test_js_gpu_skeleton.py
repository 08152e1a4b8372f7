"""GPU: the Node.js host's thinning (js/test/test_skeleton_gpu.js): Volume.skeleton, its info, burn, within, volume and profile, the pass cap,
the form without the tile cull and Volume.centreline on 70 x 19 x 11 (noise, overlapping balls), a row and one voxel, uint8 and uint16, the
three modes, equal the plain-JS statement of the contract (js/vpt/skeleton.js, which tests/test_skeleton_host.py holds to the numpy
statement); and RenderingContext({skeleton}) ends with the texels of the numpy statement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DIMS = (16, 16, 28)                                               # [depth][height][width]


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_host_thins_like_the_contract(tmp_path):
    import vpt_amd
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_skeleton_gpu.js"), str(tmp_path / "out.raw")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert res.returncode == 0 and "js skeleton gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    n = int(np.prod(DIMS))
    assert len(got) == 2 * n
    v = np.frombuffer(got[:n], np.uint8).reshape(DIMS)
    want = vpt_amd.skeleton_texels(v, 128, 255, 'ends', 0, 2)
    kept = int((want != 2).sum())
    assert 2 <= kept < int((v >= 128).sum()), "degenerate input"
    assert got[n:] == want.tobytes(), "RenderingContext({skeleton}) texels (Node host) differ from the numpy statement"
