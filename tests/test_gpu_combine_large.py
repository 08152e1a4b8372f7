"""GPU: the two-volume operations past 2^31 and 2^32 voxels (vpt_volume_combine, vpt_volume_compare): only here can a 32-bit voxel index or
byte offset in an elementwise kernel show.  The file follows tests/test_gpu_large_volumes.py: sparse volumes whose content lies in thin slabs
at z = 0, around voxel 2^31 and at the far end (tests/large_volumes.py), expected texels from the numpy statement on the small twins, a
stated peak of device memory and a skip with both figures where it is not free.

Both operations are elementwise, so a slab needs no halo: the twins' slabs are the expected texels of the volumes' slabs, and every voxel
between them is the image of background 0 in both sources."""
import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.combine import STATS, combine_texels, compare_stats

from large_volumes import TIER_A, TIER_B, Layout, voxels, volume_bytes, sparse_volume
from test_gpu_large_volumes import require, tier, hold, background, refused

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(180)
def test_mask_of_more_than_2_32_voxels(gpu_ctx):
    """MASK at tier B, odd nx, R8.  Peak: two sources and the result, three R8 volumes, 59.6 GiB.  Code 0 is outside the range, so the
    background of the result is `fill`.  The same pair is what vpt_volume_compare refuses: its voxel count is named."""
    shape = TIER_B['odd']
    n = tier(shape, 1 << 32)
    require(3 * volume_bytes(shape, 1))
    lay = Layout(shape, 2, 1)
    blocks_a, blocks_b = lay.noise(np.uint8, 101), lay.noise(np.uint8, 131)
    a = sparse_volume(gpu_ctx, lay, blocks_a)
    try:
        b = sparse_volume(gpu_ctx, lay, blocks_b)
        try:
            refused(lambda: a.compare(b), str(n), "2^32 - 1")
            out = a.mask(b, 64, 255, fill=7)
        finally:
            b.destroy()
    finally:
        a.destroy()
    try:
        want = combine_texels(lay.twin(blocks_a), lay.twin(blocks_b), 'mask', lo=64, hi=255, fill=7)
        for z_lo, z_hi, t_lo in lay.windows():                    # a result that is all fill, or a copy of a, cannot pass
            slab = want[t_lo:t_lo + (z_hi - z_lo)]
            assert 0.1 < (slab == 7).mean() < 0.9
        hold(out, want, lay.windows(), "mask R8 odd")
        background(out, lay.between(), 7, "mask")
    finally:
        out.destroy()


@pytest.mark.timeout(180)
def test_compare_with_counts_above_2_31(gpu_ctx):
    """compare at tier A (between 2^31 and 2^32 voxels), odd nx, R8.  Peak: two R8 volumes, 21.2 GiB.  Both ranges hold code 0, so the
    background, more than 2^31 voxels, is counted in in_a, in_b and both, and in nothing else: the sums are those of the slabs."""
    shape = TIER_A['odd']
    n = tier(shape, 1 << 31, 1 << 32)
    require(2 * volume_bytes(shape, 1))
    lay = Layout(shape, 2, 1)
    blocks_a, blocks_b = lay.noise(np.uint8, 151), lay.noise(np.uint8, 171)
    a = sparse_volume(gpu_ctx, lay, blocks_a)
    try:
        b = sparse_volume(gpu_ctx, lay, blocks_b)
        try:
            got = a.compare(b, (0, 100), (0, 50))
            again = a.compare(b, (0, 100), (0, 50))
            narrow = a.compare(b, (1, 100), (1, 50))              # code 0 left out: the slabs alone
        finally:
            b.destroy()
    finally:
        a.destroy()
    slabs_a, slabs_b = np.concatenate(blocks_a), np.concatenate(blocks_b)
    slabs = compare_stats(slabs_a, slabs_b, (0, 100), (0, 50))    # Python integers over the slabs' voxels
    rest = n - slabs_a.size                                       # background voxels: A = B = 0
    assert rest > 1 << 31
    want = dict(slabs, voxels=n, in_a=slabs['in_a'] + rest, in_b=slabs['in_b'] + rest, both=slabs['both'] + rest)
    assert 0 < slabs['differing'] < slabs_a.size and slabs['sum_sq'] > slabs['sum_abs'] > slabs['differing'] and slabs['max_abs'] == 255
    assert {k: got[k] for k in STATS} == {k: want[k] for k in STATS}
    assert min(got['in_a'], got['in_b'], got['both']) > 1 << 31
    assert again == got, "two runs differ"
    assert got['mse'] == want['sum_sq'] / n and got['dice'] == 2 * want['both'] / (want['in_a'] + want['in_b'])
    only = compare_stats(slabs_a, slabs_b, (1, 100), (1, 50))
    assert {k: narrow[k] for k in STATS} == dict({k: only[k] for k in STATS}, voxels=n)
