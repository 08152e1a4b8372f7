"""GPU: the Node.js host's quasi-cubic filter (js/test/test_quasicubic_gpu.js) renders MIP and MCM frames byte-equal to the Python host's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_host_quasicubic_frames_equal_the_python_hosts(gpu_ctx, tmp_path):
    import vpt_amd
    from vpt_amd.scene import Transform, Node, default_camera
    from vpt_amd.synthetic import sphere_volume, colour_tf, GoldenRatioRng
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    W, H, dims = 72, 52, (23, 18, 21)
    vol, tf = sphere_volume(0, noise=50.0, dims=dims), colour_tf(64)
    (tmp_path / "vol.raw").write_bytes(vol.tobytes()); (tmp_path / "tf.raw").write_bytes(tf.tobytes())
    args = [str(tmp_path / "vol.raw"), str(tmp_path / "tf.raw"), str(tmp_path / "out.raw"), W, H, dims[2], dims[1], dims[0]]
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_quasicubic_gpu.js")] + [str(a) for a in args],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert res.returncode == 0 and "js quasicubic gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    gvol = vpt_amd.Volume.from_array(gpu_ctx, vol, 'quasicubic')
    want = []
    for cls in (vpt_amd.MIPRenderer, vpt_amd.MCMRenderer):
        r = cls(gpu_ctx, gvol, default_camera(W / H), None, {'resolution': (W, H), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
        r.setTransferFunction(tf)
        if cls is vpt_amd.MCMRenderer:
            r.extinction = 40
        r.reset()
        for _ in range(3):
            r.render()
        want.append(np.ascontiguousarray(r.getTexture()).tobytes())
        r.destroy()
    gvol.destroy()
    assert len(got) == 2 * 8 * W * H
    assert got[:8 * W * H] == want[0], "MIP frame (Node host) differs from the Python host's"
    assert got[8 * W * H:] == want[1], "MCM frame (Node host) differs from the Python host's"
    assert len(set(want[0])) > 8                          # (the frame is not empty)
