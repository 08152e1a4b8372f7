"""GPU: the Node.js host's graph of a voxel set (js/test/test_graph_gpu.js): Volume.graph and Skeleton.graph, their info, branch and node
records, the branches and nodes as Components, classes, prune and profile on sparse noise in 70 x 10 x 6, a diagonal line and a Y through a
tile corner, one voxel and the empty set, uint8 and uint16, equal the plain-JS statement of the contract (js/vpt/graph.js, which
tests/test_graph_host.py holds to the numpy statement); and Volume.centreline with prune ends with the texels of the numpy statement."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
DIMS = (11, 19, 70)                                               # [depth][height][width]


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_node_host_builds_graphs_like_the_contract(tmp_path):
    from vpt_amd.graph import centreline_texels
    from vpt_amd.skeleton import skeleton_texels
    addon = os.path.join(ROOT, "js", "addon", "vpt_native.node")
    assert os.path.exists(addon), "build the addon first: make -C js/addon (or __graft_entry__.build())"
    res = subprocess.run([NODE, os.path.join(ROOT, "js", "test", "test_graph_gpu.js"), str(tmp_path / "out.raw")],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    assert res.returncode == 0 and "js graph gpu ok" in res.stdout.decode(), res.stdout.decode()
    got = (tmp_path / "out.raw").read_bytes()
    n = int(np.prod(DIMS))
    assert len(got) == 2 * n
    v = np.frombuffer(got[:n], np.uint8).reshape(DIMS)
    want = centreline_texels(v, 128, 255, 'ends', prune=30, prune_rounds=2)
    plain = skeleton_texels(v, 128, 255, 'ends')
    assert 2 <= int((want != 0).sum()) < int((plain != 0).sum()), "degenerate input: the pruning drops nothing"
    assert got[n:] == want.tobytes(), "centreline with prune (Node host) differs from the numpy statement"
