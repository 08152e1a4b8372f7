"""GPU: the Node.js host's distance transform (js/test/test_distance_gpu.js): the squared distances, the info and the within / channel
texels of uint8 and uint16 volumes, Volume.margin and Volume.core equal the plain-JS twins (which tests/test_distance_host.py holds to the
numpy statement), and RenderingContext({window, distance: channel}) ends with the texels of the numpy chain."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_host_transforms_like_the_contract(tmp_path):
    import vpt_amd
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_distance_gpu.js"), str(tmp_path / "out.raw")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert res.returncode == 0 and "js distance gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    dims = (21, 19, 23)
    n = 2 * int(np.prod(dims))
    ct = np.frombuffer(got[:n], '<i2').reshape(dims)
    value = vpt_amd.window_texels(ct, -200, 400, 8)
    d2 = vpt_amd.distance_squared_texels(value, 250, 254)
    pair = vpt_amd.channel_texels(value, d2, 64)
    assert len(np.unique(d2)) >= 8 and (pair[..., 1] == 255).any() and ((pair[..., 1] > 0) & (pair[..., 1] < 255)).any(), "degenerate input"
    assert got[n:] == pair.tobytes(), "RenderingContext({window, distance: channel}) texels (Node host) differ from the numpy chain"
