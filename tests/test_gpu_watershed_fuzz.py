"""GPU: fixed-seed draws of a watershed behind another volume operation (a rank filter, a window, h-minima or h-maxima, as
tests/test_gpu_reconstruct_fuzz.py chains the reconstruction): shape up to 70 x 20 x 10 (two tiles along x, three along y and z), format,
connectivity, polarity, domain and min_voxels are drawn; the volume the front step makes is read back whole and must equal its numpy
statement byte for byte, and the basins' ranks and list must equal vpt_amd.watershed_texels of it word for word.  No draw is skipped:
draw() makes only calls the contract takes.

VPT_WATERFUZZ_SEEDS=a:b widens the sweep."""
import os

import numpy as np
import pytest

from vpt_amd.rank import rank_texels
from vpt_amd.reconstruct import geodesic_texels
from vpt_amd.watershed import watershed_texels
from vpt_amd.window import window_texels

from test_gpu_pyramid import upload, whole
from test_gpu_reconstruct_fuzz import same, texels

pytestmark = pytest.mark.gpu

_SEEDS = range(*[int(v) for v in os.environ.get("VPT_WATERFUZZ_SEEDS", "0:40").split(":")])
CONSTANT = 0xBA51


def draw(seed):
    """the chain of a seed: {'source', 'front': (name, kwargs), 'call': kwargs of the watershed with the domain as fractions of M}"""
    rng = np.random.default_rng(CONSTANT + 7919 * seed)
    def axis(most):                                               # 1 .. most; three times in four at least 3, so that the volume has an inside
        n = int(rng.integers(1, most + 1))
        return int(rng.integers(3, most + 1)) if n < 3 and rng.integers(0, 4) else n
    shape = (axis(10), axis(20), axis(70))                        # [depth][height][width]
    dtype = (np.uint8, np.uint16)[int(rng.integers(0, 2))]
    M = int(np.iinfo(dtype).max)
    case = {'seed': seed, 'source': texels(rng, shape, dtype, ('noise', 'levels', 'blobs')[int(rng.integers(0, 3))])}
    front = ('rank', 'window', 'hmin', 'hmax')[int(rng.integers(0, 4))]
    if front == 'rank':
        case['front'] = ('rank', {'op': ('median', 'erode', 'dilate', 'open', 'close')[int(rng.integers(0, 5))], 'passes': 1})
    elif front == 'window':
        lo = int(rng.integers(0, M // 2))
        case['front'] = ('window', {'lo': lo, 'hi': int(rng.integers(lo + 1, M + 1)), 'bits': (8, 16)[int(rng.integers(0, 2))]})
    else:
        case['front'] = (front, {'h_fraction': float(rng.uniform(0.0, 0.3)), 'connectivity': (6, 18, 26)[int(rng.integers(0, 3))]})
    lo = float(rng.uniform(0.0, 0.4)) if rng.integers(0, 2) else 0.0
    hi = float(rng.uniform(0.6, 1.0)) if rng.integers(0, 2) else 1.0
    case['call'] = {'lo_fraction': lo, 'hi_fraction': hi, 'polarity': ('minima', 'maxima')[int(rng.integers(0, 2))],
                    'connectivity': (6, 18, 26)[int(rng.integers(0, 3))], 'min_voxels': (1, 1, 2, 9)[int(rng.integers(0, 4))]}
    return case


def describe(case):
    return "seed %d: %s %s, %s %r, then watershed %r" % (case['seed'], case['source'].dtype, case['source'].shape[::-1], case['front'][0], case['front'][1],
                                                        case['call'])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("seed", _SEEDS)
def test_a_drawn_chain_equals_its_numpy_statements(gpu_ctx, seed):
    case = draw(seed)
    what = describe(case)
    source = case['source']
    vols, basins = [upload(gpu_ctx, source)], None
    try:
        name, kw = case['front']
        if name == 'rank':
            front, want = vols[0].rank(kw['op'], kw['passes']), rank_texels(source, kw['op'], kw['passes'])
        elif name == 'window':
            front, want = vols[0].window(kw['lo'], kw['hi'], 'r%d' % kw['bits']), window_texels(source, kw['lo'], kw['hi'], kw['bits'])
        else:
            h = int(kw['h_fraction'] * int(np.iinfo(source.dtype).max))
            front, want = vols[0].geodesic(name, h, kw['connectivity']), geodesic_texels(source, name, h, kw['connectivity'])
        vols.append(front)
        same(whole(front), want, what + "\nthe front step")
        M = int(np.iinfo(want.dtype).max)
        kw = case['call']
        lo, hi = int(kw['lo_fraction'] * M), int(kw['hi_fraction'] * M)
        basins = front.watershed(lo, hi, kw['polarity'], kw['connectivity'], kw['min_voxels'])
        ranks, listed = watershed_texels(want, lo, hi, kw['polarity'], kw['connectivity'], kw['min_voxels'])
        same(basins.ranks(), ranks, what)
        assert basins.list() == listed, what
        assert basins.info['foreground_voxels'] == np.count_nonzero((want >= lo) & (want <= hi)), what
        same(whole(front), want, what + "\nthe source afterwards")
    finally:
        if basins is not None:
            basins.destroy()
        for v in vols:
            v.destroy()
