"""GPU: the Node.js host's 16-bit normalised volumes (js/test/test_norm16_gpu.js): a manifest loads only once the context has enabled
EXT_texture_norm16, and its MIP, EAM and MCM frames are byte-equal to the Python host's for the same texels."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
@pytest.mark.timeout(300)
@pytest.mark.parametrize("signed", [False, True])
def test_node_host_norm16_frames_equal_the_python_hosts(gpu_ctx, tmp_path, signed):
    import vpt_amd
    from vpt_amd.scene import Transform, Node, default_camera
    from vpt_amd.synthetic import sphere_volume, colour_tf, GoldenRatioRng
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    W, H, dims = 72, 52, (23, 18, 21)
    vol = sphere_volume(0, noise=50.0, dims=dims).astype(np.int64) * 257 + np.random.default_rng(3).integers(0, 257, size=dims)
    vol = np.clip(vol, 0, 65535)
    vol = (vol - 32768).astype(np.int16) if signed else vol.astype(np.uint16)
    tf = colour_tf(64)
    (tmp_path / "vol.raw").write_bytes(vol.astype(vol.dtype.newbyteorder('<')).tobytes()); (tmp_path / "tf.raw").write_bytes(tf.tobytes())
    args = [str(tmp_path / "vol.raw"), str(tmp_path / "tf.raw"), str(tmp_path / "out.raw"), W, H, dims[2], dims[1], dims[0], int(signed)]
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_norm16_gpu.js")] + [str(a) for a in args],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert res.returncode == 0 and "js norm16 gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    gvol = vpt_amd.Volume.from_array(gpu_ctx, vol, 'linear', norm16=True)
    want = []
    for cls in (vpt_amd.MIPRenderer, vpt_amd.EAMRenderer, vpt_amd.MCMRenderer):
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
    assert len(got) == 3 * 8 * W * H
    for k, name in enumerate(('MIP', 'EAM', 'MCM')):
        assert got[k * 8 * W * H:(k + 1) * 8 * W * H] == want[k], "%s frame (Node host) differs from the Python host's" % name
    assert len(set(want[0])) > 8                          # (the frame is not empty)
