"""GPU: per-component measurements and set selection past 2^31 voxels (vpt_components_measure, vpt_components_keep_set): only here can a
32-bit voxel index or a 32-bit plane offset in the measuring kernel or in the set emitter show.

The volume is tier A 'odd' of tests/large_volumes.py (811 x 809 x 4096, about 2.7 G voxels: the largest 32-bit ranks admit), content in four
thin slabs, one of them around voxel 2^31 and one at the far end.  The expected records come from the twin: a component lies within one
slab, so against the twin's record sum_z differs by voxels * (z0 - twin z0), min_z and max_z by that offset, and every other field is equal
(tests/test_measure_host.py shows that on a small shape).  Skips, with both figures, when less device memory is free than the peak."""
import numpy as np
import pytest

import vpt_amd
from vpt_amd.measure import MEASURE_DTYPE

from large_volumes import TIER_A, Layout, volume_bytes, field_bytes, sparse_volume
from test_gpu_large_volumes import require, tier, hold, background

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(180)
def test_measure_and_keep_set_of_more_than_2_31_voxels(gpu_ctx):
    """R8, 6-connected components of the top sixteenth of the codes: 277 154 small components over the four slabs.  Peak, computed as
    tests/test_gpu_large_volumes.py computes it: source 10.6 + handle 12.5 + the count array 10.0 = 33.1 GiB while labelling; measuring adds
    88 + 4 bytes a record to the handle's 12.5 GiB; keep_set holds handle 12.5 + result 10.6 = 23.1 GiB.  Measured on an MI355X (the
    smallest free-memory figure a sampling thread saw during each step): 33.3, 12.7 and 23.3 GiB."""
    shape = TIER_A['odd']
    n = tier(shape, 1 << 31, 0xFFFFFFFE)
    nx, ny, nz = shape
    require(max(volume_bytes(shape, 1) + field_bytes(shape, 1) + 4 * n, field_bytes(shape, 1) + volume_bytes(shape, 1)))
    lo, M = 240, 255
    lay = Layout(shape, 2, 1, marks=(1 << 30, 1 << 31))
    blocks = lay.noise(np.uint8, 211)
    twin = lay.twin(blocks)
    ranks, listed = vpt_amd.components_texels(twin, lo, M, 6)
    want = vpt_amd.measure_texels(ranks, twin, 0, len(listed))
    # every component lies within one slab: its planes move by the slab's offset
    offset = np.array([lay.to_volume(int(z)) - int(z) for z in want['min_z']], np.uint64)
    assert (np.array([lay.to_volume(int(z)) - int(z) for z in want['max_z']], np.uint64) == offset).all()
    want['sum_z'] += want['voxels'] * offset
    want['min_z'] += offset.astype(np.uint32); want['max_z'] += offset.astype(np.uint32)
    far = (want['min_z'].astype(np.uint64) * ny + want['min_y']) * nx + want['min_x'] > (1 << 31)
    assert len(listed) >= 1000 and len(set(offset.tolist())) == 4 and far.sum() >= 100 and int(want['sum_z'].max()) > 1 << 12
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        found = src.components(lo, M, 6)
    finally:
        src.destroy()
    try:
        assert found.list() == [(x, y, lay.to_volume(z), v) for x, y, z, v in listed]
        got = found.measure()
        for name in MEASURE_DTYPE.names:
            bad = np.flatnonzero(got[name] != want[name])
            assert len(bad) == 0, "%d records differ in %s, first %d: %d, expected %d" % (len(bad), name, bad[0], got[name][bad[0]], want[name][bad[0]])
        first = len(listed) - 7                                       # a window at the list's end: the smallest components, in every slab
        assert found.measure(first, 7).tobytes() == want[first:].tobytes()
        chosen = np.flatnonzero(far)[::2] + 1                         # half of the components beyond voxel 2^31 ...
        chosen = np.concatenate([chosen, np.arange(1, len(listed) + 1, 5)])      # ... and every fifth of all
        kept = found.keep_set(chosen.tolist(), 3)
        try:
            hold(kept, vpt_amd.keep_set_texels(twin, ranks, chosen.tolist(), 3), lay.windows(), "keep_set")
            background(kept, lay.between(), 3, "keep_set")
        finally:
            kept.destroy()
    finally:
        found.destroy()
