"""GPU: forty seeded random cases of the isosurface mesh (vpt_volume_surface): dimensions 1 .. 40 x 1 .. 12 x 1 .. 8, a format (R8, RG8,
R16, RG16), a channel, a level and content (noise, blobs, all equal), each held byte for byte to vpt_amd.surface.surface_texels."""
import numpy as np
import pytest

from test_gpu_surface import check

pytestmark = pytest.mark.gpu

CASES = 40


def draw(seed):
    """(array, level, channel, scan_words) of case `seed`"""
    rng = np.random.default_rng(7000 + seed)
    w, h, d = int(rng.integers(1, 41)), int(rng.integers(1, 13)), int(rng.integers(1, 9))
    dtype = (np.uint8, np.uint16)[int(rng.integers(0, 2))]
    channels = int(rng.integers(1, 3))
    channel = int(rng.integers(0, channels))
    M = int(np.iinfo(dtype).max)
    level = (1, M, int(rng.integers(1, M + 1)), int(rng.integers(1, M + 1)))[int(rng.integers(0, 4))]
    content = ('noise', 'blobs', 'equal')[int(rng.integers(0, 3))]
    shape = (d, h, w) + ((2,) if channels == 2 else ())
    if content == 'noise':
        a = rng.integers(0, M + 1, shape, dtype=dtype)
    elif content == 'equal':
        a = np.full(shape, (0, level - 1, level, M)[int(rng.integers(0, 4))], dtype)
    else:
        z, y, x = np.indices((d, h, w)).astype(np.float64)
        field = np.zeros((d, h, w))
        for _ in range(int(rng.integers(1, 5))):
            c, r = rng.random(3) * (d, h, w), 1.0 + rng.random() * 6.0
            field = np.maximum(field, 1.0 - np.sqrt((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / r)
        one = np.clip(np.rint(level + field * M * 0.5 - M * 0.1), 0, M).astype(dtype)
        a = np.stack([one, one[::-1, ::-1, ::-1]], axis=3) if channels == 2 else one
    scan_words = (None, None, 1, 7)[int(rng.integers(0, 4))]
    return np.ascontiguousarray(a), level, channel, scan_words


def test_the_draws_cover_the_ground():
    """(no device) the forty draws hold every format, both channels, the extreme levels, every content and a capped scan"""
    seen = set()
    for seed in range(CASES):
        a, level, channel, scan_words = draw(seed)
        M = int(np.iinfo(a.dtype).max)
        seen |= {(a.dtype.name, a.ndim), 'channel %d' % channel, 'level 1' if level == 1 else 'level M' if level == M else 'level',
                 'capped' if scan_words else 'default', 'flat' if a.min() == a.max() else 'varied'}
    assert {('uint8', 3), ('uint8', 4), ('uint16', 3), ('uint16', 4), 'channel 0', 'channel 1', 'level 1', 'level M', 'level', 'capped', 'default',
            'flat', 'varied'} <= seen


@pytest.mark.parametrize('seed', range(CASES))
def test_fuzz(gpu_ctx, seed):
    a, level, channel, scan_words = draw(seed)
    check(gpu_ctx, a, level, channel, scan_words)
