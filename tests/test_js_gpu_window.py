"""GPU: the Node.js host's value-range window (js/test/test_window_gpu.js): a signed 16-bit RAW volume through RAWReader({bits: 16, signed});
its range, percentile window and code histogram, the windowed texels (R8 and R16) and the MIP and MCM frames of the windowed volume,
directly and through RenderingContext({window}), are byte-equal to the contract's (vpt_amd.window_texels) and to the Python host's."""
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
def test_node_host_windows_and_renders_like_the_python_host(gpu_ctx, tmp_path):
    import vpt_amd
    from vpt_amd.scene import Transform, Node, default_camera
    from vpt_amd.synthetic import sphere_volume, colour_tf, GoldenRatioRng
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    W, H, dims = 72, 52, (23, 19, 21)
    d, h, w = dims
    vol = (sphere_volume(0, noise=45.0, dims=dims).astype(np.int64) * 4000 // 255 - 1000).astype('<i2')      # Hounsfield-like
    tf = colour_tf(64, 48)
    (tmp_path / "vol.raw").write_bytes(vol.tobytes()); (tmp_path / "tf.raw").write_bytes(tf.tobytes())
    args = [str(tmp_path / "vol.raw"), str(tmp_path / "tf.raw"), str(tmp_path / "out.raw"), W, H, w, h, d, 64, 48]
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_window_gpu.js")] + [str(a) for a in args],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert res.returncode == 0 and "js window gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    hist = np.bincount(vol.astype(np.int64).reshape(-1) + 32768, minlength=65536).astype(np.uint32)
    pw = vpt_amd.percentile_window(hist, 2, 98, True)
    numbers = np.array([vol.min(), vol.max(), pw[0], pw[1]], np.float64)
    t8, t16 = vpt_amd.window_texels(vol, -200, 400, 8), vpt_amd.window_texels(vol, -200, 400, 16)
    assert len(np.unique(t8)) >= 32
    chains = []
    for lo, hi in ((int(vol.min()), int(vol.max())), pw):
        wt = vpt_amd.window_texels(vol, lo, hi, 16)
        chains.append(np.ascontiguousarray(np.stack([wt, vpt_amd.gradient_magnitude(wt, 'central', 1)], axis=-1)))
    frame = 8 * W * H
    sizes = [numbers.nbytes, hist.nbytes, t8.nbytes, t16.nbytes, frame, frame, frame, frame, chains[0].nbytes, chains[1].nbytes]
    assert len(got) == sum(sizes)
    parts, o = [], 0
    for n in sizes:
        parts.append(got[o:o + n]); o += n
    assert parts[0] == numbers.tobytes(), "range / percentile window (Node host): %s" % np.frombuffer(parts[0], np.float64)
    assert parts[1] == hist.tobytes(), "code histogram (Node host)"
    assert parts[2] == t8.tobytes(), "readBlock of the R8 window (Node host) differs from the contract"
    assert parts[3] == t16.tobytes(), "readBlock of the R16 window (Node host) differs from the contract"
    src = vpt_amd.Volume.from_array(gpu_ctx, vol.astype(np.int16), norm16=True)
    wvol = src.window(-200, 400)
    src.destroy()
    want = []
    for cls in (vpt_amd.MIPRenderer, vpt_amd.MCMRenderer):
        r = cls(gpu_ctx, wvol, default_camera(W / H), None, {'resolution': (W, H), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
        r.reset()                                         # (the Node script resets twice, as RenderingContext.chooseRenderer + the caller do)
        r.setTransferFunction(tf)
        if cls is vpt_amd.MCMRenderer:
            r.extinction = 40
        r.reset()
        for _ in range(3):
            r.render()
        want.append(np.ascontiguousarray(r.getTexture()).tobytes())
        r.destroy()
    wvol.destroy()
    assert parts[4] == want[0], "MIP frame (Node host) differs from the Python host's"
    assert parts[5] == want[1], "MCM frame (Node host) differs from the Python host's"
    assert parts[6] == want[0], "MIP frame through RenderingContext({window}) (Node host)"
    assert parts[7] == want[1], "MCM frame through RenderingContext({window}) (Node host)"
    assert parts[8] == chains[0].tobytes(), "RenderingContext({window: 'range', gradient}) texels (Node host)"
    assert parts[9] == chains[1].tobytes(), "RenderingContext({window: {percentiles}, gradient}) texels (Node host)"
    assert len(set(want[0])) > 8                          # (the frame is not empty)
