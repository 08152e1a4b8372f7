"""GPU: the Node.js host's reconstruction and geodesic operations (js/test/test_reconstruct_gpu.js): Volume.reconstruct (both ops, a
two-channel marker), Volume.geodesic (all seven) and the timed and capped forms on three shapes, uint8 and uint16, equal the plain-JS twin of
the contract (js/vpt/reconstruct.js, which tests/test_reconstruct_host.py holds to the numpy statement); and RenderingContext({rank, geodesic,
smooth}) ends with the texels of the numpy chain, in the Node host and in the Python host."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DIMS = (13, 22, 37)                                               # [depth][height][width]


def chain(v):
    """rank 'median', geodesic hmax with h = 40 under 18, smooth 1"""
    import vpt_amd
    flattened = vpt_amd.geodesic_texels(vpt_amd.rank_texels(v, 'median', 1), 'hmax', 40, 18)
    return vpt_amd.smooth_texels(flattened, 1)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_host_reconstructs_like_the_contract(tmp_path):
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_reconstruct_gpu.js"), str(tmp_path / "out.raw")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert res.returncode == 0 and "js reconstruct gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    n = int(np.prod(DIMS))
    assert len(got) == 2 * n
    v = np.frombuffer(got[:n], np.uint8).reshape(DIMS)
    assert got[n:] == chain(v).tobytes(), "RenderingContext({rank, geodesic, smooth}) texels (Node host) differ from the numpy chain"


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_python_rendering_context_applies_the_geodesic_option_behind_rank_and_in_front_of_smooth():
    import vpt_amd
    from vpt_amd.readers import RAWReader
    rng = np.random.default_rng(77)
    v = rng.integers(0, 256, size=DIMS, dtype=np.uint8)
    for spec, want in (({'op': 'hmax', 'h': 40, 'connectivity': 18}, chain(v)),
                       ({'op': 'fill_holes'}, vpt_amd.smooth_texels(vpt_amd.geodesic_texels(vpt_amd.rank_texels(v, 'median', 1), 'fill_holes', 0, 6), 1))):
        rc = vpt_amd.RenderingContext({'resolution': (72, 52), 'rank': 'median', 'geodesic': spec, 'smooth': 1})
        try:
            rc.setVolume(RAWReader(v, {'width': DIMS[2], 'height': DIMS[1], 'depth': DIMS[0]}))
            assert rc.volume.read_block(0, 0, 0, DIMS[2], DIMS[1], DIMS[0]).tobytes() == want.tobytes(), spec
            assert want.tobytes() != vpt_amd.smooth_texels(vpt_amd.rank_texels(v, 'median', 1), 1).tobytes(), "degenerate input"
        finally:
            rc.destroy()
