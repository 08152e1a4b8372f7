"""GPU: connected components of a volume large enough for every streaming kernel's grid-stride loop to go round a second time.

stream_grid (vpt_volume_components.hip) caps k_merge, k_flatten, k_sizes, k_census, k_compact, k_ranks, k_read_field, k_select and k_pair at
8192 workgroups of 256 threads: the loop `i += gridDim.x * 256` wraps above 2 097 152 items, and the emitters, four voxels an item, above
8 388 608 voxels.  The forms to doubt are the wave-granular ones: `base` of k_sizes and k_compact, whose ballot and shuffle must see whole
waves on the wrapped step too, and the emitters' tail `quads * 4 + t0` behind a wrapped loop of quads.  The other shapes of the suite stay
below 20 000 voxels.  Held to the numpy statement byte for byte as everywhere; the statement takes seconds at this size and is taken once
per case."""
import numpy as np
import pytest

import vpt_amd

from components_model import at_least
from test_gpu_components import check, differences, noise, noise_range, statement
from test_gpu_pyramid import upload, whole

pytestmark = pytest.mark.gpu

WRAP = (129, 255, 257)                                              # nx, ny, nz: 8 454 015 voxels


def test_the_shape_wraps_every_loop():
    nx, ny, nz = WRAP
    n = nx * ny * nz
    assert n // 4 > 8192 * 256 and n % 4 == 3 and nx % 4 != 0 and n % 64 != 0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype, connectivity, seed", ((np.uint8, 6, 101), (np.uint16, 26, 103)))
def test_noise_on_a_wrapped_grid_equals_the_contract(gpu_ctx, dtype, connectivity, seed):
    nx, ny, nz = WRAP
    M = int(np.iinfo(dtype).max)
    a = noise(dtype, WRAP, seed)
    lo, hi = noise_range(dtype, connectivity)
    assert dtype != np.uint8 or (lo, hi) == (0, 76)
    want = statement(a, lo, hi, connectivity)
    ranks, listed = check(gpu_ctx, a, lo, hi, connectivity, what='wrap', want=want)
    sizes = [c[3] for c in listed]
    assert len(listed) >= 64, "degenerate input: %d components" % len(listed)
    assert len(set(sizes[:255])) < len(sizes[:255]), "degenerate input: no size tie"
    assert 2 * sizes[0] < sum(sizes), "degenerate input: one component holds half of the foreground"
    assert len(listed) > 8192 * 256 // 64 and int(ranks.max()) > M, "degenerate input: fewer roots than waves, or G does not saturate"
    # min_voxels = 2: the slots of k_compact with holes where the dropped roots are
    ranks2, stay = at_least(ranks, listed, 2)
    assert 64 <= len(stay) <= len(listed) - 64
    check(gpu_ctx, a, lo, hi, connectivity, 2, what='wrap, min 2', want=(ranks2, stay, len(listed)))
    # a selection, and a box of ranks that is not a run of whole slices and holds more texels than one trip of k_read_field
    src = upload(gpu_ctx, a)
    found = src.components(lo, hi, connectivity)
    out = found.keep(2, 3, 7)
    differences(whole(out), vpt_amd.keep_texels(a, ranks, 2, 3, 7), 'wrap: keep(2, 3, 7)')
    x, y, z, w, h, d = 1, 1, 1, nx - 1, ny - 1, 200
    assert w * h * d > 8192 * 256
    differences(found.ranks(x, y, z, w, h, d), np.ascontiguousarray(ranks[z:z + d, y:y + h, x:x + w]), 'wrap: a box of ranks')
    assert found.profile()[1:] == (1, 1)                            # noise: no chain of tile components comes near the production caps
    for thing in (out, found, src):
        thing.destroy()
