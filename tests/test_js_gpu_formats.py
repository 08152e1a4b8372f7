"""GPU: the Node.js host's SNORM and packed-format volumes (js/test/test_formats_gpu.js) against their R32F / RG32F twins."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_host_snorm_and_packed_formats():
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_formats_gpu.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = res.stdout.decode()
    assert res.returncode == 0, out
    assert "js formats gpu ok" in out
