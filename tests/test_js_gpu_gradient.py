"""GPU: the Node.js host's gradient-magnitude channel (js/test/test_gradient_gpu.js): the derived volume's texels and histogram equal the
contract's (vpt_amd.gradient_magnitude), and its MIP and MCM frames, directly and through RenderingContext({gradient}), are byte-equal to
the Python host's."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_host_derives_reads_back_and_renders_like_the_python_host(gpu_ctx, tmp_path):
    import vpt_amd
    from vpt_amd.scene import Transform, Node, default_camera
    from vpt_amd.synthetic import sphere_volume, colour_tf, GoldenRatioRng
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    W, H, dims = 72, 52, (23, 19, 21)
    d, h, w = dims
    vol, tf = sphere_volume(0, noise=45.0, dims=dims), colour_tf(64, 48)
    (tmp_path / "vol.raw").write_bytes(vol.tobytes()); (tmp_path / "tf.raw").write_bytes(tf.tobytes())
    args = [str(tmp_path / "vol.raw"), str(tmp_path / "tf.raw"), str(tmp_path / "out.raw"), W, H, w, h, d, 64, 48]
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_gradient_gpu.js")] + [str(a) for a in args],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert res.returncode == 0 and "js gradient gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    pair = np.ascontiguousarray(np.stack([vol, vpt_amd.gradient_magnitude(vol, 'sobel', 4)], axis=-1))
    assert len(np.unique(pair[..., 1])) >= 32
    box = np.ascontiguousarray(pair[3:14, 2:11, 1:14])
    hist = np.histogram2d(pair[..., 1].reshape(-1), pair[..., 0].reshape(-1), bins=[np.arange(257), np.arange(257)])[0].astype(np.uint32)
    frame = 8 * W * H
    sizes = [pair.nbytes, box.nbytes, hist.nbytes, frame, frame, frame, frame]
    assert len(got) == sum(sizes)
    parts, o = [], 0
    for n in sizes:
        parts.append(got[o:o + n]); o += n
    assert parts[0] == pair.tobytes(), "readBlock of the derived volume (Node host) differs from the contract"
    assert parts[1] == box.tobytes(), "readBlock of a box (Node host)"
    assert parts[2] == hist.tobytes(), "histogram (Node host)"
    src = vpt_amd.Volume.from_array(gpu_ctx, vol)
    gvol = src.derive_gradient('sobel', 4)
    src.destroy()
    want = []
    for cls in (vpt_amd.MIPRenderer, vpt_amd.MCMRenderer):
        r = cls(gpu_ctx, gvol, default_camera(W / H), None, {'resolution': (W, H), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
        r.reset()                                         # (the Node script resets twice, as RenderingContext.chooseRenderer + the caller do)
        r.setTransferFunction(tf)
        if cls is vpt_amd.MCMRenderer:
            r.extinction = 40
        r.reset()
        for _ in range(3):
            r.render()
        want.append(np.ascontiguousarray(r.getTexture()).tobytes())
        r.destroy()
    gvol.destroy()
    assert parts[3] == want[0], "MIP frame (Node host) differs from the Python host's"
    assert parts[4] == want[1], "MCM frame (Node host) differs from the Python host's"
    assert parts[5] == want[0], "MIP frame through RenderingContext({gradient}) (Node host)"
    assert parts[6] == want[1], "MCM frame through RenderingContext({gradient}) (Node host)"
    assert len(set(want[0])) > 8                          # (the frame is not empty)
