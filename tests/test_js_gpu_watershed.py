"""GPU: the Node.js host's watershed (js/test/test_watershed_gpu.js): Volume.watershed (both polarities, a two-channel relief, texels given),
the timed and capped forms and Volume.split on three shapes, uint8 and uint16, equal the plain-JS twin of the contract (js/vpt/watershed.js,
which tests/test_watershed_host.py holds to the numpy statement); and RenderingContext({split}) ends with the texels of the numpy chain, in
the Node host and in the Python host."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DIMS = (16, 16, 28)                                               # [depth][height][width]: the worked example's grid


def chain(v):
    """(value, min(rank of the basin, 255)) of split(100, 255) with the option's defaults"""
    import vpt_amd
    return vpt_amd.label_texels(v, vpt_amd.split_texels(v, 100, 255)[0])


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_host_floods_like_the_contract(tmp_path):
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_watershed_gpu.js"), str(tmp_path / "out.raw")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert res.returncode == 0 and "js watershed gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    n = int(np.prod(DIMS))
    assert len(got) == 3 * n
    v = np.frombuffer(got[:n], np.uint8).reshape(DIMS)
    want = chain(v)
    assert set(np.unique(want[..., 1])) == {0, 1, 2}, "degenerate input"
    assert got[n:] == want.tobytes(), "RenderingContext({split}) texels (Node host) differ from the numpy chain"


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_python_rendering_context_applies_the_split_option():
    import vpt_amd
    from vpt_amd.readers import RAWReader
    from reconstruct_cases import two_balls
    v = two_balls(19)
    for spec, want in (({'lo': 100, 'hi': 300}, chain(v)),                                   # hi is open above
                       ({'lo': 100, 'hi': 255, 'h': 0, 'steps': 2, 'connectivity': 6, 'minVoxels': 900},
                        vpt_amd.label_texels(v, vpt_amd.split_texels(v, 100, 255, 0, 2, 6, 900)[0]))):
        rc = vpt_amd.RenderingContext({'resolution': (72, 52), 'split': spec})
        try:
            rc.setVolume(RAWReader(v, {'width': DIMS[2], 'height': DIMS[1], 'depth': DIMS[0]}))
            assert rc.volume.native_format()[0] == vpt_amd._native.FORMAT_RG8
            assert rc.volume.read_block(0, 0, 0, DIMS[2], DIMS[1], DIMS[0]).tobytes() == want.tobytes(), spec
            assert len(np.unique(want[..., 1])) >= 2, "degenerate input"
        finally:
            rc.destroy()
