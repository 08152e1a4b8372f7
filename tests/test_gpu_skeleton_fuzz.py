"""GPU: fixed-seed draws of the thinning (vpt_volume_skeleton) against vpt_amd.skeleton_burn_texels, word for word and field for field.
Every axis is in 1 .. 24; the fill is white noise of density 0.3 .. 0.8 or thresholded smoothed noise (blobs); format, value range, mode
and pass cap are drawn.  Every eighth case also runs with the tile cull switched off.

VPT_SKELFUZZ_SEEDS=a:b widens the sweep."""
import os

import numpy as np
import pytest

from vpt_amd.skeleton import MODES, skeleton_burn_texels

from test_gpu_pyramid import upload
from test_gpu_skeleton import same

pytestmark = pytest.mark.gpu

_SEEDS = range(*[int(v) for v in os.environ.get("VPT_SKELFUZZ_SEEDS", "0:40").split(":")])
CONSTANT = 0x5CE1


def smoothed(rng, shape):
    """noise averaged over 3 x 3 x 3 boxes twice (the border repeated), cut at its median: blobs"""
    field = rng.random(shape)
    for _ in range(2):
        padded = np.pad(field, 1, mode='edge')
        field = sum(padded[dz:dz + shape[0], dy:dy + shape[1], dx:dx + shape[2]] for dz in range(3) for dy in range(3) for dx in range(3)) / 27.0
    return field >= np.median(field)


def draw(seed):
    rng = np.random.default_rng(CONSTANT + 7919 * seed)
    shape = tuple(int(rng.integers(1, 25)) for _ in range(3))                 # [depth][height][width]
    dtype = (np.uint8, np.uint16)[int(rng.integers(2))]
    M = int(np.iinfo(dtype).max)
    lo = int(rng.integers(1, M))                                              # 1 .. M - 1
    hi = int(rng.integers(lo, M)) if rng.integers(2) else M - 1               # lo .. M - 1: 0 and M are outside the range
    kind = ('noise', 'blobs')[int(rng.integers(2))]
    mask = rng.random(shape) < rng.uniform(0.3, 0.8) if kind == 'noise' else smoothed(rng, shape)
    inside = rng.integers(lo, hi + 1, size=shape)
    below, above = rng.integers(0, lo, size=shape), rng.integers(hi + 1, M + 1, size=shape)
    texels = np.where(mask, inside, np.where(rng.random(shape) < 0.5, below, above)).astype(dtype)
    return {'seed': seed, 'texels': texels, 'lo': lo, 'hi': hi, 'kind': kind, 'mode': list(MODES)[int(rng.integers(3))],
            'passes': int(rng.integers(0, 5)), 'object': int(mask.sum())}


def describe(case):
    return "seed %d: %s %s %s, [%d, %d] %s passes %d" % (case['seed'], case['kind'], case['texels'].dtype, case['texels'].shape[::-1], case['lo'], case['hi'],
                                                         case['mode'], case['passes'])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("seed", _SEEDS)
def test_a_drawn_thinning_equals_its_numpy_statement(gpu_ctx, seed):
    case = draw(seed)
    what = describe(case)
    a = case['texels']
    want, info = skeleton_burn_texels(a, case['lo'], case['hi'], case['mode'], case['passes'])
    assert info['object_voxels'] == case['object'], what
    v = upload(gpu_ctx, a)
    try:
        for flags in ((None, 1) if seed % 8 == 0 else (None,)):
            k = v.skeleton(case['lo'], case['hi'], case['mode'], case['passes'], _flags=flags)
            try:
                same(k.burn(), want, what + "\nflags %r" % (flags,))
                assert k.info == info, what
            finally:
                k.destroy()
    finally:
        v.destroy()


def test_the_draws_cover_the_ground():
    cases = [draw(seed) for seed in range(40)]
    assert {c['mode'] for c in cases} == set(MODES) and {c['kind'] for c in cases} == {'noise', 'blobs'}
    assert {c['texels'].dtype for c in cases} == {np.dtype(np.uint8), np.dtype(np.uint16)} and {c['passes'] for c in cases} == {0, 1, 2, 3, 4}
    assert sum(c['object'] > 100 for c in cases) >= 20
