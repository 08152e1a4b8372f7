"""GPU: the Node.js host's resampling (js/test/test_resample_gpu.js): Volume.resample (filtered and nearest) and Volume.isotropic of uint8
and uint16 volumes read back equal to the plain-JS twin of the contract (js/vpt/resample.js, which tests/test_resample_host.py holds to the
numpy statement), and RenderingContext({window, resample, rank, smooth, gradient}) ends with the texels of the numpy chain."""
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
def test_node_host_resamples_like_the_contract(tmp_path):
    import vpt_amd
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_resample_gpu.js"), str(tmp_path / "out.raw")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert res.returncode == 0 and "js resample gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    dims = (23, 19, 21)
    n = 2 * int(np.prod(dims))
    ct = np.frombuffer(got[:n], '<i2').reshape(dims)
    windowed = vpt_amd.window_texels(ct, -200, 400, 16)
    nx, ny, nz = vpt_amd.isotropic_shape((21, 19, 23), (0.7, 0.7, 1.6))
    assert (nx, ny, nz) == (21, 19, 53)
    grid = vpt_amd.resample_texels(windowed, (nz, ny, nx))
    value = vpt_amd.smooth_texels(vpt_amd.rank_texels(grid, 'median', 1), 1)
    pair = np.ascontiguousarray(np.stack([value, vpt_amd.gradient_magnitude(value, 'sobel', 2)], axis=-1))
    assert len(np.unique(value)) >= 32
    assert got[n:] == pair.tobytes(), "RenderingContext({window, resample, rank, smooth, gradient}) texels (Node host) differ from the numpy chain"
