"""GPU: the Node.js host's surface (js/test/test_surface_gpu.js): Volume.surface, its info, vertices, quads (whole and paged), the capped
scan, both channels of a two-channel volume, uint8 and uint16, the empty result, the mesh measures and the writers equal the plain-JS
statement of the contract (js/vpt/surface.js, which tests/test_js_surface_host.py holds to the numpy statement); and the vertices and
quads of one noise volume, written to a file, equal the numpy statement's bytes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DIMS = (6, 11, 37)                                                # [depth][height][width]


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_host_extracts_like_the_contract(tmp_path):
    from vpt_amd.surface import surface_texels
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_surface_gpu.js"), str(tmp_path / "out.raw")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert res.returncode == 0 and "js surface gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    n = int(np.prod(DIMS))
    texels = np.frombuffer(got[:n], np.uint8).reshape(DIMS)
    v, q = surface_texels(texels, 128)
    assert len(v) > 1000
    assert got[n:] == v.tobytes() + q.tobytes(), "the surface of the Node host differs from the numpy statement"
