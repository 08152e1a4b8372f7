"""GPU: the watershed of a volume large enough for the grid-stride loops of its streaming kernels to go round a second time.

stream_grid caps k_ws_merge and k_ws_channel (and the components' tail behind them) at 8192 workgroups of 256 threads: the loop
`i += gridDim.x * 256` wraps above 2 097 152 voxels.  The other shapes of the suite stay below 40 000 voxels.  Held to the numpy statement
word for word as everywhere; the statement takes seconds at this size and is taken once per case."""
import numpy as np
import pytest

from vpt_amd.components import keep_texels
from vpt_amd.watershed import watershed_texels

from test_gpu_pyramid import upload, whole

pytestmark = pytest.mark.gpu

WRAP = (129, 127, 129)                                              # nx, ny, nz: 2 113 407 voxels


def test_the_shape_wraps_the_loops():
    nx, ny, nz = WRAP
    assert nx * ny * nz > 8192 * 256 and nx % 64 != 0 and ny % 8 != 0 and nz % 4 != 0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype, channels, connectivity, polarity, seed", ((np.uint8, 1, 6, 'minima', 201), (np.uint16, 2, 6, 'maxima', 203)))
def test_noise_on_a_wrapped_grid_equals_the_contract(gpu_ctx, dtype, channels, connectivity, polarity, seed):
    nx, ny, nz = WRAP
    M = int(np.iinfo(dtype).max)
    rng = np.random.default_rng(seed)
    # noise over 24 codes: plateaus of a few voxels, basins across every tile face
    a = (rng.integers(0, 24, size=(nz, ny, nx) + ((2,) if channels == 2 else ())) * (M // 23)).astype(dtype)
    channel = channels - 1
    lo, hi = M // 23, M
    want_ranks, want_list = watershed_texels(a, lo, hi, polarity, connectivity, 2, channel)
    assert len(want_list) >= 64, "degenerate input: %d basins" % len(want_list)
    v = upload(gpu_ctx, a)
    basins = v.watershed(lo, hi, polarity, connectivity, 2, channel)
    try:
        got = basins.ranks()
        bad = np.argwhere(got != want_ranks)
        assert len(bad) == 0, "%d ranks differ, first at %s: %d, expected %d" % (len(bad), bad[0], got[tuple(bad[0])], want_ranks[tuple(bad[0])])
        assert basins.list() == want_list
        relief = a[..., channel] if channels == 2 else a
        kept = basins.keep(1, 50)                                   # the snapshot: the chosen channel, copied by a wrapped loop
        assert np.array_equal(whole(kept), keep_texels(relief, want_ranks, 1, 50))
        kept.destroy()
    finally:
        basins.destroy()
        v.destroy()
