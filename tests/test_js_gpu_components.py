"""GPU: the Node.js host's connected components (js/test/test_components_gpu.js): the ranks, the list, the info and the keep / label texels
of uint8 and uint16 volumes equal the plain-JS twins (which tests/test_components_host.py holds to the numpy statement), and
RenderingContext({rank, components}) in both modes ends with the texels of the numpy chain."""
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
def test_node_host_labels_like_the_contract(tmp_path):
    import vpt_amd
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_components_gpu.js"), str(tmp_path / "out.raw")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert res.returncode == 0 and "js components gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    dims = (23, 19, 21)
    n = int(np.prod(dims))
    a = np.frombuffer(got[:n], np.uint8).reshape(dims)
    m = vpt_amd.rank_texels(a, 'median')
    ranks, listed = vpt_amd.components_texels(m, 0, 76, 6, 2)
    assert len(listed) >= 16
    kept = vpt_amd.keep_texels(m, ranks, 1, 3)
    assert kept.tobytes() != m.tobytes(), "the selection changes nothing"
    assert got[n:2 * n] == kept.tobytes(), "RenderingContext({rank, components: keep}) texels (Node host) differ from the numpy chain"
    ranks, listed = vpt_amd.components_texels(m, 0, 80, 18, 2)
    assert len(listed) >= 16
    assert got[2 * n:] == vpt_amd.label_texels(m, ranks).tobytes(), "RenderingContext({rank, components: label}) texels (Node host) differ from the numpy chain"
