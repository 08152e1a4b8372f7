"""GPU: the Node.js host's HDR environment maps (js/test/test_envmap_gpu.js): the same .hdr file, read by js/vpt/hdr.js and set as the
environment of MCM and MCS, gives frames byte-equal to the Python host's (vpt_amd.hdr.read_hdr); short buffers are refused."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_hdr_host import encode_hdr, rgbe_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
@pytest.mark.timeout(300)
def test_node_host_hdr_frames_equal_the_python_hosts(gpu_ctx, tmp_path):
    import vpt_amd
    from vpt_amd.scene import Transform, Node, default_camera
    from vpt_amd.synthetic import sphere_volume, colour_tf, GoldenRatioRng
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    W, H, dims = 96, 64, (23, 18, 21)
    vol = sphere_volume(0, noise=50.0, dims=dims)
    tf = colour_tf(64)
    img = rgbe_image(16, 32, seed=12)
    img[..., 3] = 127 + img[..., 3] % 12                           # radiance up to 2^3
    (tmp_path / "vol.raw").write_bytes(vol.tobytes()); (tmp_path / "tf.raw").write_bytes(tf.tobytes())
    (tmp_path / "sky.hdr").write_bytes(encode_hdr(img, magic=b"#?RGBE", extra=(b"EXPOSURE=4",)))
    args = [tmp_path / "vol.raw", tmp_path / "tf.raw", tmp_path / "sky.hdr", tmp_path / "out.raw", W, H, dims[2], dims[1], dims[0]]
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_envmap_gpu.js")] + [str(a) for a in args],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert res.returncode == 0 and "js envmap gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    env = vpt_amd.read_hdr(str(tmp_path / "sky.hdr"))
    gvol = vpt_amd.Volume.from_array(gpu_ctx, vol, 'linear')
    want = []
    for cls in (vpt_amd.MCMRenderer, vpt_amd.MCSRenderer):
        r = cls(gpu_ctx, gvol, default_camera(W / H), env, {'resolution': (W, H), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
        r.setTransferFunction(tf)
        r.extinction = 40 if cls is vpt_amd.MCMRenderer else 9
        r.reset()
        for _ in range(3):
            r.render()
        want.append(np.ascontiguousarray(r.getTexture()).tobytes())
        r.destroy()
    gvol.destroy()
    assert len(got) == 2 * 8 * W * H
    for k, name in enumerate(('MCM', 'MCS')):
        assert got[k * 8 * W * H:(k + 1) * 8 * W * H] == want[k], "%s frame (Node host) differs from the Python host's" % name
    assert np.frombuffer(want[0], np.float16).max() > 1.0          # (HDR light reached the image)
