"""GPU: the Node.js host's local thickness (js/test/test_thickness_gpu.js): Distance.thickness, its emitters, the timed and flagged forms,
Volume.thickness and Volume.openBall on 9 x 13 x 21 and on a ball cut by the border, uint8 and uint16, equal the plain-JS statement of the
contract (js/vpt/thickness.js, which tests/test_thickness_host.py holds to the numpy statement); and RenderingContext({thickness}) ends with
the texels of the numpy chain, in the Node host and in the Python host."""
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
def test_node_host_measures_thickness_like_the_contract(tmp_path):
    import vpt_amd
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_thickness_gpu.js"), str(tmp_path / "out.raw")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert res.returncode == 0 and "js thickness gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    n = int(np.prod(DIMS))
    assert len(got) == 3 * n
    v = np.frombuffer(got[:n], np.uint8).reshape(DIMS)
    want = vpt_amd.thickness_texels(v, 128, 255)
    assert set(np.unique(want[..., 1])) >= {0, 8, 12}, "degenerate input"       # the two diameters, floor(2 sqrt(17)) and floor(2 sqrt(37))
    assert got[n:] == want.tobytes(), "RenderingContext({thickness}) texels (Node host) differ from the numpy chain"


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_python_rendering_context_applies_the_thickness_option():
    import vpt_amd
    from vpt_amd.readers import RAWReader
    from test_gpu_thickness import ball
    rng = np.random.default_rng(8)
    mask = ball(DIMS, (8, 8, 9), 6) | ball(DIMS, (8, 8, 19), 4)
    v = np.where(mask, rng.integers(128, 256, size=DIMS), rng.integers(0, 128, size=DIMS)).astype(np.uint8)
    d2 = vpt_amd.distance_squared_texels(v, 128, 255, 'rest')
    pore = vpt_amd.thickness_squared_texels(vpt_amd.distance_squared_texels(v, 128, 255, 'range'))
    for spec, want, fmt in (({'lo': 128, 'hi': 300, 'mode': 'channel'}, vpt_amd.thickness_texels(v, 128, 255), 'RG8'),               # hi is open above
                            ({'lo': 128, 'hi': 255, 'mode': 'channel', 'steps': 5, 'seeds': 'range'}, vpt_amd.channel_texels(v, pore, 5), 'RG8'),
                            ({'lo': 128, 'hi': 255, 'mode': 'within', 'from': 26, 'fill': 3}, vpt_amd.open_ball_texels(v, 128, 255, 5, 3), 'R8')):
        rc = vpt_amd.RenderingContext({'resolution': (72, 52), 'thickness': spec})
        try:
            rc.setVolume(RAWReader(v, {'width': DIMS[2], 'height': DIMS[1], 'depth': DIMS[0]}))
            assert rc.volume.native_format()[0] == getattr(vpt_amd._native, 'FORMAT_' + fmt)
            assert rc.volume.read_block(0, 0, 0, DIMS[2], DIMS[1], DIMS[0]).tobytes() == want.tobytes(), spec
            assert len(np.unique(want)) >= 3, "degenerate input"
        finally:
            rc.destroy()
    assert int(d2.max()) > 25                                     # the opening by the ball of radius 5 keeps something
