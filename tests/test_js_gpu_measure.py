"""GPU: the Node.js host's per-component measurements and set selection (js/test/test_measure_gpu.js): Components.measure (windows, values
of the other width, a two-channel volume) and Components.keepSet (a subset, a boolean mask, the empty set, an interval against keep) on one
noise volume per width and on the 3-D checkerboard equal the plain-JS twin of the contract (js/vpt/measure.js, which
tests/test_measure_host.py holds to the numpy statement)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_host_measures_like_the_contract():
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_measure_gpu.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert res.returncode == 0 and "js measure gpu ok" in res.stdout.decode(), res.stdout.decode()
