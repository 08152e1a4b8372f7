"""GPU: the Node.js host's two-volume operations (js/test/test_combine_gpu.js): Volume.combine (every op, a two-channel second volume, a
mask of the other width) and Volume.compare of uint8 and uint16 volumes equal the plain-JS twin of the contract (js/vpt/combine.js, which
tests/test_combine_host.py holds to the numpy statement), and RenderingContext({combine, rank, smooth}) with a reader for a second volume
on another grid ends with the texels of the numpy chain."""
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
def test_node_host_combines_like_the_contract(tmp_path):
    import vpt_amd
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_combine_gpu.js"), str(tmp_path / "out.raw")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert res.returncode == 0 and "js combine gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    dims, other = (23, 19, 21), (9, 11, 13)
    n, k = int(np.prod(dims)), int(np.prod(other))
    assert len(got) == 2 * n + k
    v = np.frombuffer(got[:n], np.uint8).reshape(dims)
    m = np.frombuffer(got[n:n + k], np.uint8).reshape(other)
    masked = vpt_amd.combine_texels(v, vpt_amd.resample_texels(m, dims, 'nearest'), 'mask', lo=64, hi=255, fill=2)
    assert 0.05 < (masked != v).mean() < 0.95, "degenerate input"
    value = vpt_amd.smooth_texels(vpt_amd.rank_texels(masked, 'median', 1), 1)
    assert len(np.unique(value)) >= 32
    assert got[n + k:] == value.tobytes(), "RenderingContext({combine, rank, smooth}) texels (Node host) differ from the numpy chain"
