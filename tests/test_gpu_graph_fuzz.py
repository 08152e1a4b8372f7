"""GPU: a short fuzz of the graph unit (vpt_volume_graph): random shapes up to 80 x 20 x 12, random densities from a few voxels to sets that are
mostly nodes, both texel widths, every record, rank, class and two prunings byte for byte against the numpy statement (vpt_amd.graph).  The
seeds are fixed: a failure names its case."""
import numpy as np
import pytest

from vpt_amd import graph as G

from test_gpu_pyramid import upload, whole

pytestmark = pytest.mark.gpu

CASES = list(range(12))


def draw(case):
    rng = np.random.default_rng(7000 + case)
    shape = (int(rng.integers(1, 13)), int(rng.integers(1, 21)), int(rng.integers(1, 81)))
    density = float(rng.choice([0.02, 0.05, 0.08, 0.12, 0.2, 0.35]))
    dtype = (np.uint8, np.uint16)[case % 2]
    M = int(np.iinfo(dtype).max)
    lo = int(rng.integers(1, M // 2))
    hi = int(rng.integers(M // 2, M))                              # codes remain on both sides of the range
    kept = rng.random(shape) < density
    outside = np.where(rng.random(shape) < 0.5, rng.integers(0, lo, size=shape), rng.integers(hi + 1, M + 1, size=shape))
    a = np.where(kept, rng.integers(lo, hi + 1, size=shape), outside).astype(dtype)
    assert np.array_equal((a >= lo) & (a <= hi), kept)
    return a, lo, hi


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", CASES)
def test_random_sets_equal_the_statement(gpu_ctx, case):
    a, lo, hi = draw(case)
    want = G.graph_texels(a, lo, hi)
    what = "case %d: %s %s [%d, %d], %d kept" % (case, a.shape, a.dtype, lo, hi, want['info']['kept_voxels'])
    v = upload(gpu_ctx, a)
    g = v.graph(lo, hi)
    branches, nodes = g.branches, g.nodes
    try:
        assert g.info == want['info'], what
        assert g.branch_records().tobytes() == want['branches'].tobytes(), what
        assert g.node_records().tobytes() == want['nodes'].tobytes(), what
        assert branches.ranks().tobytes() == want['branch_ranks'].tobytes() and nodes.ranks().tobytes() == want['node_ranks'].tobytes(), what
        pair = g.classes()
        assert whole(pair).tobytes() == G.classes_texels(a, want).tobytes(), what
        pair.destroy()
        for length, debris, fill in ((24, False, 0), (60, True, int(a.max()))):
            out = g.prune(length, debris=debris, fill=fill)
            assert whole(out).tobytes() == G.prune_texels(a, want, length, flags=G.PRUNE_DEBRIS if debris else 0, fill=fill).tobytes(), (what, length)
            out.destroy()
    finally:
        branches.destroy(); nodes.destroy(); g.destroy(); v.destroy()
